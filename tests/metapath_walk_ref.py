"""NumPy restatement of the sampled meta-path neighbours (han_metapath_walk_*, include/han_hip.h): the walks on
tests/rng_ref.han_rand64, the visit counts per start row, and the fanout cut.  The GPU tests compare the kernels with it
bit for bit; tests/test_metapath_walk_host.py checks it against scipy products and the exact transition
probabilities."""
import numpy as np

from tests.rng_ref import han_rand64

STREAM_WALK = 3            # HAN_STREAM_WALK


def endpoints(hops, walks, seed=0, rows=None):
    """(r1 - r0, walks) int64: where walk w of start node r0 + r ends, -1 for a walk that died.  hops: a list of
    (rowptr, colidx) per hop, as stored (repeats are parallel edges)."""
    L = len(hops)
    n = len(hops[0][0]) - 1
    r0, r1 = (0, n) if rows is None else rows
    start = np.arange(r0, r1, dtype=np.int64)[:, None]
    w = np.arange(walks, dtype=np.int64)[None, :]
    cur = np.broadcast_to(start, (r1 - r0, walks)).copy()
    alive = np.ones(cur.shape, dtype=bool)
    for h, (rowptr, colidx) in enumerate(hops):
        rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
        at = np.where(alive, cur, 0)
        beg = rowptr[at]
        deg = rowptr[at + 1] - beg
        assert deg.max(initial=0) < 1 << 32
        alive &= deg > 0
        x, y = han_rand64(seed, STREAM_WALK, start & 0xFFFFFFFF, w * ((L + 1) // 2) + (h >> 1))
        r = y if h & 1 else x
        e = (r * deg.astype(np.uint64)) >> np.uint64(32)           # r < 2^32 and deg < 2^32: exact in uint64
        pos = np.where(alive, beg + e.astype(np.int64), 0)
        cur = np.where(alive, colidx[pos] if colidx.size else 0, -1)
    return np.where(alive, cur, -1)


def keep_row(cols, counts, i, fanout, diag):
    """Indices into the ascending `cols` that stay: with diag column i always, and of the others the `fanout` of
    largest count, ties to the smaller column; in column order."""
    cols, counts = np.asarray(cols), np.asarray(counts)
    other = np.nonzero(cols != i)[0] if diag else np.arange(len(cols))
    best = sorted(other.tolist(), key=lambda k: (-int(counts[k]), int(cols[k])))[:fanout]
    return np.array(sorted(best + (np.nonzero(cols == i)[0].tolist() if diag else [])), dtype=np.int64)


def sample(hops, walks, fanout=None, seed=0, diag=False, rows=None, ends=None):
    """(rowptr int64, colidx int32, visits int32) of the sampled graph: the definition of include/han_hip.h.  ends: the
    endpoints() of the same (hops, walks, seed, rows), for callers that cut them more than one way."""
    fanout = walks if fanout is None else fanout
    n = len(hops[0][0]) - 1
    r0, r1 = (0, n) if rows is None else rows
    ends = endpoints(hops, walks, seed, (r0, r1)) if ends is None else ends
    rowptr, colidx, visits = [0], [], []
    for r in range(r1 - r0):
        i = r0 + r
        cols, cnt = np.unique(ends[r][ends[r] >= 0], return_counts=True)
        if diag and i not in cols:
            at = int(np.searchsorted(cols, i))
            cols, cnt = np.insert(cols, at, i), np.insert(cnt, at, 0)
        keep = keep_row(cols, cnt, i, fanout, diag)
        colidx.append(cols[keep])
        visits.append(cnt[keep])
        rowptr.append(rowptr[-1] + len(keep))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.asarray(rowptr, dtype=np.int64), cat(colidx, np.int32), cat(visits, np.int32)


def values(visits, walks, weights):
    """The fp32 values metapath_sample stores: the visits, or visits / walks divided in fp32."""
    v = np.asarray(visits).astype(np.float32)
    return v if weights == "count" else v / np.float32(walks)
