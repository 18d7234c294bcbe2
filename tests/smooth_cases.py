"""Shared generators of the smooth-label tests (tests/test_smooth_cpu.py, tests/test_smooth_gpu.py):
seeded random maps, speckled block maps, the exhaustive 3 x 3 patterns and the geometry cases.
Everything is integer and seeded; nothing here needs a GPU."""
import functools

import numpy as np

LABELS = (0, 1, 2, 7, 255)
SPECKLE = (0, 3, 200, 255)
# (H, W, crop_h, crop_w)
CPU_GEOMETRIES = [(9, 13, 9, 13), (9, 13, 4, 5), (5, 7, 1, 1), (33, 33, 33, 31), (7, 70, 6, 67)]


def random_maps(seed: int, B: int, H: int, W: int):
    """(labels, codes) uint8 [B, H, W]: labels drawn from ``LABELS``, codes from 12 .. 255."""
    rng = np.random.default_rng(seed)
    lab = np.asarray(LABELS, np.uint8)[rng.integers(0, len(LABELS), (B, H, W))]
    return lab, rng.integers(12, 256, (B, H, W)).astype(np.uint8)


def speckled(seed: int, B: int, H: int, W: int, block: int = 4, share: float = 0.1):
    """(labels, codes) uint8 [B, H, W]: piecewise-constant maps (blocks of ``block`` pixels) with
    ``share`` of the pixels replaced by speckle, blocks and speckle drawn from ``SPECKLE``; codes
    uniform in 0 .. 255."""
    rng = np.random.default_rng(seed)
    vals = np.asarray(SPECKLE, np.uint8)
    bh, bw = -(-H // block), -(-W // block)
    lab = np.kron(vals[rng.integers(0, len(vals), (B, bh, bw))],
                  np.ones((1, block, block), np.uint8))[:, :H, :W]
    noise = vals[rng.integers(0, len(vals), (B, H, W))]
    lab = np.where(rng.random((B, H, W)) < share, noise, lab).astype(np.uint8)
    return lab, rng.integers(0, 256, (B, H, W)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def exhaustive():
    """(labels, codes) uint8 [19683, 5, 6] with a 3 x 3 crop: frame i holds the base-3 digits of
    i, every three-label 3 x 3 pattern exactly once (the centre is digit 4). The pad pixels hold
    label 9 and seeded codes: they must pass through."""
    n = 3 ** 9
    i = np.arange(n)
    lab = np.full((n, 5, 6), 9, np.uint8)
    lab[:, :3, :3] = np.stack([(i // 3 ** d) % 3 for d in range(9)], 1).reshape(n, 3, 3)
    codes = np.random.default_rng(5).integers(12, 256, (n, 5, 6)).astype(np.uint8)
    lab.setflags(write=False)
    codes.setflags(write=False)
    return lab, codes


def exhaustive_centres():
    """For the centre pixel of every pattern of ``exhaustive``, from the definition alone: (the
    output label, kept, kept on a tie, changed by the smallest-label rule on a tie), the last
    three boolean [19683]."""
    lab, _ = exhaustive()
    pat = lab[:, :3, :3].reshape(-1, 9)
    v = np.stack([(pat == c).sum(1) for c in range(3)], 1)  # votes per label
    m = v.max(1)
    own = pat[:, 4]
    kept = v[np.arange(len(pat)), own] == m
    tie = (v == m[:, None]).sum(1) > 1
    out = np.where(kept, own, (v == m[:, None]).argmax(1)).astype(np.uint8)
    return out, kept, kept & tie, ~kept & tie


def gpu_geometries(tw: int, th: int):
    """name -> (H, W, crop_h, crop_w) for a tile of ``tw`` x ``th`` pixels."""
    geo = {f"cpu{i}": g for i, g in enumerate(CPU_GEOMETRIES)}
    geo.update({
        "one_wider": (9, tw + 3, 9, tw + 1),
        "one_narrower": (9, tw + 3, 9, tw - 1),
        "one_taller": (th + 3, 13, th + 1, 13),
        "one_shorter": (th + 3, 13, th - 1, 13),
        "edge_on_tile_edge": (th + 3, tw + 3, th, tw),  # pad on both sides
    })
    return geo


def below_window():
    """(labels, codes) [1, 5, 7] with a 2 x 2 crop, smaller than any window: three pixels outvote
    the fourth at every R."""
    lab, codes = speckled(77, 1, 5, 7)
    lab = lab.copy()
    lab[0, :2, :2] = [[3, 3], [3, 200]]
    return lab, codes


def cut_cluster(tw: int):
    """(labels, codes) [1, 12, 2 tw]: a block map with a cluster of single-pixel speckles that
    the edge between the two tiles cuts."""
    lab, codes = speckled(78, 1, 12, 2 * tw, block=6, share=0.05)
    lab = lab.copy()
    for y, x, c in ((4, tw - 2, 0), (5, tw - 1, 3), (5, tw, 200), (6, tw + 1, 255), (4, tw, 3), (6, tw - 1, 200)):
        lab[0, y, x] = c
    return lab, codes
