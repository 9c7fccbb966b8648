"""Shared inputs of the live-forward tests (tests/test_live_forward_host.py, tests/test_live_forward_gpu.py): the K2
graph whose rows fall into all three sets of a degree-binned launch, and the row subsets the issue names."""
import numpy as np
import torch

K2_N = 600                 # rows = table rows
SPLIT_DEG, SPLIT_CHUNK = 64, 32      # patched into ops for this graph: the rows of 70 and 150 entries are long
LONG = {37: 70, 411: 150}            # row -> entries (3 and 5 chunks of 32)
SUBSETS = ["random", "no_short", "one_long", "single", "empty", "all"]


def k2_degrees():
    """Row lengths 0 .. 40 (every length 14 times over: 4, 15, 16, 17 and their neighbours included), then the two
    long rows."""
    deg = np.arange(K2_N) % 41
    for r, d in LONG.items():
        deg[r] = d
    return deg.astype(np.int64)


def k2_graph(device, valued=False, seed=0):
    """(rowptr int64, colidx int32, values or None) on `device`; distinct columns inside a row."""
    rng = np.random.default_rng(seed)
    deg = k2_degrees()
    cols = np.concatenate([np.sort(rng.choice(K2_N, size=int(d), replace=False)) for d in deg] + [np.zeros(0, np.int64)])
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    vals = torch.from_numpy(rng.uniform(0.5, 1.5, size=cols.size).astype(np.float32)).to(device) if valued else None
    return (torch.from_numpy(rowptr.astype(np.int64)).to(device), torch.from_numpy(cols.astype(np.int32)).to(device), vals)


def k2_subset(which, seed=1):
    """(K2_N,) bool numpy mask of the rows to compute."""
    deg = k2_degrees()
    m = np.zeros(K2_N, dtype=bool)
    if which == "random":
        m[np.random.default_rng(seed).permutation(K2_N)[:K2_N // 10]] = True
        m[37] = True                 # with one of the long rows
    elif which == "no_short":
        m[deg >= 16] = True
    elif which == "one_long":
        m[411] = True
    elif which == "single":
        m[5] = True
    elif which == "all":
        m[:] = True
    elif which != "empty":
        raise ValueError(which)
    return m


def brute_force_sets(deg, mask, short_deg, split_deg):
    """The partition of the listed rows by length: (short ids in (ceil(deg / 4), id) order, mid ids ascending, long ids
    ascending)."""
    ids = np.nonzero(mask)[0]
    short = sorted((int(i) for i in ids if deg[i] < short_deg), key=lambda i: ((int(deg[i]) + 3) // 4, i))
    mid = [int(i) for i in ids if short_deg <= deg[i] <= split_deg]
    long = [int(i) for i in ids if deg[i] > split_deg]
    return short, mid, long
