"""Shared generators of the stable-label tests (tests/test_stable_cpu.py, tests/test_stable_gpu.py):
the every-sequence planes, the flickering piecewise-constant label maps and the host oracle of
a batch layout. Everything is integer and seeded; nothing here needs a GPU."""
import numpy as np

from semantic_segmentation_server_amd.postprocess import stable as SB

GATE = 128


def every_sequence_labels():
    """uint8 [6, 27, 27]: pixel i of the 27 x 27 plane gets the base-3 digits of i over 6
    frames -- every sequence of length 6 over {0, 1, 2} exactly once (3^6 = 729 pixels)."""
    i = np.arange(27 * 27)
    return np.stack([(i // 3 ** t) % 3 for t in range(6)]).astype(np.uint8).reshape(6, 27, 27)


def every_sequence_conf(g: int = GATE):
    """(labels, codes) uint8 [4, 36, 36]: pixel i gets the base-6 digits d of i over 4 frames as
    the symbol (label d % 3, code g - 1 + d // 3) -- every sequence of length 4 over the six
    symbols exactly once (6^4 = 1296 pixels)."""
    i = np.arange(36 * 36)
    d = np.stack([(i // 6 ** t) % 6 for t in range(4)])
    return ((d % 3).astype(np.uint8).reshape(4, 36, 36),
            (g - 1 + d // 3).astype(np.uint8).reshape(4, 36, 36))


def flicker(seed: int, T: int, H: int, W: int, flip: float = 0.1, block: int = 3):
    """(labels, codes) uint8 [T, H, W]: piecewise-constant maps of labels 0 .. 255 (blocks of
    ``block`` pixels); from frame to frame about ``flip`` of the pixels take a new label, half of
    them as whole blocks, half as single pixels, so runs of a candidate of every length up to T
    occur. The codes are uniform in 0 .. 255."""
    rng = np.random.default_rng(seed)
    bh, bw = -(-H // block), -(-W // block)
    up = np.ones((block, block), np.uint8)
    cur = np.kron(rng.integers(0, 256, (bh, bw)).astype(np.uint8), up)[:H, :W].copy()
    labs = []
    for _ in range(T):
        blocks = np.kron((rng.random((bh, bw)) < flip / 2).astype(np.uint8), up)[:H, :W].astype(bool)
        new = np.kron(rng.integers(0, 256, (bh, bw)).astype(np.uint8), up)[:H, :W]
        frame = np.where(blocks, new, cur)
        keep = rng.random((H, W)) < 0.5  # half of the block flips persist: candidates that win
        cur = np.where(blocks & keep, new, cur)
        px = rng.random((H, W)) < flip / 2
        frame = np.where(px, rng.integers(0, 256, (H, W)).astype(np.uint8), frame)
        labs.append(frame.astype(np.uint8))
    return np.stack(labs), rng.integers(0, 256, (T, H, W)).astype(np.uint8)


def rows_of(counts):
    """The stream position of every row of a batch laid out by ``counts``."""
    return [s for s, n in enumerate(counts) for _ in range(n)]


class Oracle:
    """The host definition over a batch layout: ``run`` takes a batch [B, H, W] (and codes or
    None) laid out by ``counts`` and returns the stabilised planes; ``state`` is what the device
    state must hold afterwards, per stream [header | crop_h * crop_w words] as uint32."""

    def __init__(self, N, g, counts, crop_h, crop_w):
        self.st = SB.Stabilizers(N, g)
        self.counts, self.crop_h, self.crop_w = list(counts), crop_h, crop_w

    def run(self, labels, conf):
        return self.st.step(labels, conf, self.crop_w, self.crop_h, rows_of(self.counts))

    def state(self):
        n = self.crop_h * self.crop_w
        out = np.zeros((len(self.counts), 1 + n), np.uint32)
        for s in range(len(self.counts)):
            t = self.st.of(s)
            if t.started:
                out[s, 0], out[s, 1:] = 1, t.state_words()
        return out.reshape(-1)
