"""Shared cases of the zone-event tests (tests/test_events_cpu.py, tests/test_events_gpu.py):
presence rows built by hand -- the definition (postprocess/events.py) is total over any rows whose
track ids are distinct and non-zero within a frame, it does not need a dwell-consistent ``D`` --
and their oracle rows through events.py. No GPU is touched here.
"""
import numpy as np

from semantic_segmentation_server_amd.postprocess import events as EV
from semantic_segmentation_server_amd.postprocess import presence as PR

SENT = 0x5A5A5A5A
CW, CH = 40, 30
D_VALUES = np.array([0, 1, 2, 0xFFFFFFFF], np.uint32)


def row(K, R, ids, D, P=None, first=None, crop=(CW, CH)):
    """The presence words (with tracks) of one frame: ``ids`` uint32 [n], ``D`` [n, R], ``P``
    [n, R] (default: a function of the position) and ``first`` [n] (default: label 1 + a % 7, root
    the id)."""
    ids = np.asarray(ids, np.uint32).reshape(-1)
    n = len(ids)
    assert n <= K and len(set(ids.tolist())) == n and (ids != 0).all()
    D = np.asarray(D, np.uint32).reshape(n, R)
    if P is None:
        P = (1 + 3 * np.arange(n * R, dtype=np.uint32)).reshape(n, R) + ids[:, None]
    if first is None:
        first = ((1 + np.arange(n, dtype=np.uint32) % 7) << 24) | (ids & 0xFFFFFF)
    U = PR.unit(R, True)
    w = np.zeros(PR.frame_words(K, R, True), np.uint32)
    w[:4] = (n, crop[0] * crop[1], crop[0], crop[1])
    e = w[4:4 + U * n].reshape(n, U)
    e[:, 0], e[:, 1], e[:, 2:2 + R], e[:, 2 + R:] = first, ids, np.asarray(P, np.uint32).reshape(n, R), D
    return w


def random_sequence(rng, K, R, frames):
    """``frames`` rows of one stream: some ids continue from the previous frame (in a new
    order), the fresh ones are larger than any earlier id, ``D`` is drawn from {0, 1, 2,
    0xFFFFFFFF}; empty frames occur."""
    out, prev, nxt = [], np.zeros(0, np.uint32), 1
    for _ in range(frames):
        n = int(rng.integers(0, K + 1))
        keep = prev[rng.random(len(prev)) < 0.6][:n]
        fresh = np.arange(nxt, nxt + n - len(keep), dtype=np.uint32)
        nxt += len(fresh)
        ids = rng.permutation(np.concatenate([keep, fresh]).astype(np.uint32))
        D = D_VALUES[rng.integers(0, 4, (n, R))]
        P = rng.integers(0, 1 << 24, (n, R)).astype(np.uint32)
        out.append(row(K, R, ids, D, P))
        prev = ids
    return out


def oracle(rows, R, E, prev=None):
    """The event rows of one stream's consecutive presence rows (``prev``: the row before the
    first, None: none), sentinel-free: every word defined."""
    out = []
    for w in rows:
        out.append(EV.events_between(prev, w, R, E))
        prev = w
    return out


def all_flip(K, R):
    """(prev, cur): every entry of prev leaves every row (its track ends: cur's ids are all new)
    and every entry of cur enters every row: K R LEAVEs, then K R ENTERs."""
    prev = row(K, R, np.arange(1, K + 1), np.full((K, R), 7, np.uint32))
    cur = row(K, R, np.arange(K + 1, 2 * K + 1), np.ones((K, R), np.uint32))
    return prev, cur


def events_at(K, R, pn, cn, candidates):
    """(prev, cur) with ``pn`` and ``cn`` entries whose events are exactly the given candidate
    indices (LEAVE slots (b, r) = divmod(c, R) for c < pn R, then ENTER slots). The tracks of the
    first min(pn, cn) entries continue, in reversed order; nothing else is an event: prev.D is 2
    and cur.D is 3 elsewhere."""
    m = min(pn, cn)
    pid = np.arange(1, pn + 1, dtype=np.uint32)
    cid = np.concatenate([pid[:m][::-1], np.arange(pn + 1, pn + 1 + cn - m, dtype=np.uint32)])
    pD = np.full((pn, R), 2, np.uint32)
    pD[m:] = 0                      # a track without a successor: quiet unless asked for
    cD = np.full((cn, R), 3, np.uint32)
    used = set()
    for c in sorted(set(int(c) for c in candidates)):
        assert 0 <= c < (pn + cn) * R
        if c < pn * R:
            b, r = divmod(c, R)
            if b < m:
                cell = (m - 1 - b, r)
                assert cell not in used
                used.add(cell)
                cD[cell] = 0
            else:
                pD[b, r] = 5
        else:
            a, r = divmod(c - pn * R, R)
            assert (a, r) not in used
            used.add((a, r))
            cD[a, r] = 1
    return row(K, R, pid, pD), row(K, R, cid, cD)


def boundary_candidates(pn, cn, R):
    """The scan's lane, wave and LEAVE / ENTER boundaries among the candidates."""
    total = (pn + cn) * R
    return sorted({c for c in (0, 63, 64, 255, 256, pn * R - 1, pn * R, total - 1) if 0 <= c < total})
