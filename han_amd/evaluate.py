"""Downstream evaluation of ``final_embed`` (the step after the hot path):
``jhyexp.py:20-86`` restated -- KNN (k=5) macro/micro-F1 over train fractions
0.2/0.4/0.6/0.8 x 10 shuffles, and KMeans NMI/ARI x 10.  CPU, scikit-learn, as in
the reference (``ex_acm3025.py:279-291``); it returns the scores instead of only
printing them.

With ``device=`` given, ``my_KNN`` / ``my_Kmeans`` run on the GPU instead (the ``han_knn_topk`` / ``han_knn_vote``
/ ``han_contingency`` / ``han_kmeans_step`` kernels behind ``knn_classify``, ``f1_scores``, ``nmi_ari`` and
``kmeans``): the embeddings stay on the device and only the small count tables come back.  The scores are formed
on the host in float64 from those tables (``f1_from_table``, ``nmi_ari_from_table``: scikit-learn's conventions).

``data/exp.py:25-62`` is the reference's second copy of the clustering evaluation; it adds the silhouette score of
the k-means labels (``data/exp.py:46-49``).  ``silhouette_samples`` / ``silhouette_score`` are that number on the
host (scikit-learn) or on the device (``han_silhouette``), and ``my_Kmeans(..., silhouette=True)`` is that form.

Both evaluation modules of the reference import ``sklearn.manifold`` (``jhyexp.py:16``, ``data/exp.py:20``) for the
t-SNE picture of the embeddings; ``tsne`` is scikit-learn's exact t-SNE on the host or ``han_tsne_calibrate`` /
``han_tsne_step`` on the device.

Random streams: the reference draws its shuffles from NumPy's GLOBAL legacy generator
(``np.random.permutation``, jhyexp.py:33) and lets scikit-learn's KMeans fall back on the
same global generator (``random_state=None``, jhyexp.py:62).  Here both use ONE
``np.random.RandomState(seed)`` -- the same bit stream as ``np.random.seed(seed)`` followed
by the reference's calls -- so a seeded run reproduces the reference's numbers exactly
(tests/golden/jhyexp_ref.npz holds outputs of the reference's own functions)."""
from __future__ import annotations

import numpy as np


def my_KNN(x, y, k=5, split_list=(0.2, 0.4, 0.6, 0.8), time=10, shuffle=True, seed=None, verbose=True, device=None):
    """jhyexp.py:20-51.  x (n,d) embeddings, y (n,) labels or one-hot (n,c).
    Returns {split: (macro_f1, micro_f1)} averaged over `time` repetitions.
    device=None: scikit-learn on the host, as the reference.  With a device: the same permutations from the same
    RandomState -- hence the same splits --, scored by knn_classify / f1_scores on the GPU."""
    if device is not None:
        return _my_knn_device(x, y, k, split_list, time, shuffle, seed, verbose, device)
    from sklearn.metrics import f1_score
    from sklearn.neighbors import KNeighborsClassifier
    rng = np.random.RandomState(seed) if not isinstance(seed, np.random.RandomState) else seed
    x = np.squeeze(np.array(x))
    y = np.array(y)
    if y.ndim > 1:
        y = np.argmax(y, axis=1)
    out = {}
    for ss in split_list:
        split = int(x.shape[0] * ss)
        macro, micro = [], []
        for _ in range(time):
            if shuffle:                      # the reference re-permutes the SAME arrays each time (:32-35)
                perm = rng.permutation(x.shape[0])
                x, y = x[perm, :], y[perm]
            est = KNeighborsClassifier(n_neighbors=k).fit(x[:split], y[:split])
            pred = est.predict(x[split:])
            macro.append(f1_score(y[split:], pred, average="macro"))
            micro.append(f1_score(y[split:], pred, average="micro"))
        out[ss] = (float(np.mean(macro)), float(np.mean(micro)))
        if verbose:
            print("KNN({}avg, split:{}, k={}) f1_macro: {:.4f}, f1_micro: {:.4f}".format(
                time, ss, k, out[ss][0], out[ss][1]))
    return out


def my_Kmeans(x, y, k=4, time=10, seed=None, verbose=True, device=None, silhouette=False):
    """jhyexp.py:54-86.  Returns (NMI, ARI) averaged over `time` fits.
    device=None: scikit-learn on the host, as the reference.  With a device: `time` fits of kmeans() (k-means++
    seeding, Lloyd on the GPU) drawing from ONE RandomState, scored by nmi_ari; the random stream is not
    scikit-learn's, so the clusterings are equally good, not identical.
    silhouette=True is the data/exp.py:25-54 form: (NMI, ARI, silhouette), the third the silhouette_score of each
    fit's labels averaged likewise.  It draws nothing from the RandomState, so NMI and ARI do not depend on it."""
    if device is not None:
        return _my_kmeans_device(x, y, k, time, seed, verbose, device, silhouette)
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    from sklearn.metrics import silhouette_score as sk_silhouette_score
    x = np.squeeze(np.array(x))
    y = np.array(y)
    if y.ndim > 1:
        y = np.argmax(y, axis=1)
    nmi, ari, sil = [], [], []
    rs = np.random.RandomState(seed) if not isinstance(seed, np.random.RandomState) else seed
    est = KMeans(n_clusters=k, random_state=rs)          # ONE estimator, library defaults (jhyexp.py:62)
    for i in range(time):
        pred = est.fit(x, y).predict(x)                  # re-fitted `time` times (jhyexp.py:67-68)
        nmi.append(normalized_mutual_info_score(y, pred))
        ari.append(adjusted_rand_score(y, pred))
        if silhouette:                                   # data/exp.py:47-48
            sil.append(sk_silhouette_score(x, est.labels_, metric="euclidean"))
    return _kmeans_result(nmi, ari, sil, silhouette, verbose)


def _kmeans_result(nmi, ari, sil, silhouette, verbose):
    res = float(np.mean(nmi)), float(np.mean(ari))
    if silhouette:
        res += (float(np.mean(sil)),)
    if verbose:                                          # jhyexp.py:86 / data/exp.py:54
        print(("NMI (10 avg): {:.4f} , ARI (10avg): {:.4f}, silhouette(10avg): {:.4f}" if silhouette else
               "NMI (10 avg): {:.4f} , ARI (10avg): {:.4f}").format(*res))
    return res


# ----------------------------------------------------------------------------------------------------------------
# The GPU path
# ----------------------------------------------------------------------------------------------------------------
KNN_MAX_K = 16          # han_knn_topk
KMEANS_MAX_K = 64       # han_kmeans_step


def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "device")


def _pick_device(device, *arrays):
    import torch
    if device is not None:
        return torch.device(device)
    for a in arrays:
        if _is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda")


def _embed(a, device):
    """An (n, d) fp32 matrix on the device: a GPU tensor is used as it is, anything else is copied once."""
    import torch
    t = a if _is_tensor(a) else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    t = t.to(device=device, dtype=torch.float32)
    return t if t.stride(-1) == 1 else t.contiguous()


def _labels(a, device):
    """(n,) int32 class ids on the device (one-hot rows are reduced by argmax)."""
    import torch
    if not _is_tensor(a):
        a = np.asarray(a)
        if a.ndim > 1:
            a = np.argmax(a, axis=1)
        a = torch.as_tensor(np.ascontiguousarray(a.astype(np.int32)))
    elif a.dim() > 1:
        a = a.argmax(dim=1)
    return a.to(device=device, dtype=torch.int32).contiguous()


def _shape2(a, name):
    shp = tuple(a.shape)
    if len(shp) != 2:
        raise ValueError(f"{name}: expected an (n, d) matrix, got shape {shp}")
    return shp


def knn_classify(x_train, y_train, x_test, k=5, device=None):
    """KNeighborsClassifier(n_neighbors=k).fit(x_train, y_train).predict(x_test) on the GPU: brute-force neighbours
    under the total order (distance, train index) and a majority vote with ties to the smallest class id.
    Returns the (n_test,) int32 predictions as a tensor on the device."""
    n_train, d = _shape2(x_train, "x_train")
    n_test, d_test = _shape2(x_test, "x_test")
    if isinstance(k, bool) or int(k) != k or k < 1 or k > KNN_MAX_K:
        raise ValueError(f"k = {k!r}: expected an integer in [1, {KNN_MAX_K}]")
    if k > n_train:
        raise ValueError(f"k = {k} neighbours of {n_train} train rows")
    if d != d_test:
        raise ValueError(f"x_train has width {d}, x_test {d_test}")
    if tuple(y_train.shape)[0] != n_train:
        raise ValueError(f"y_train: {tuple(y_train.shape)[0]} labels for {n_train} rows")
    from . import ops
    dev = _pick_device(device, x_train, x_test)
    idx, _ = ops.knn_topk(_embed(x_test, dev), _embed(x_train, dev), int(k))
    return ops.knn_vote(idx, _labels(y_train, dev))


def _table(y_true, y_pred, ca=None, cb=None):
    from . import ops
    dev = _pick_device(None, y_true, y_pred)
    a, b = _labels(y_true, dev), _labels(y_pred, dev)
    if a.shape != b.shape:
        raise ValueError(f"{tuple(a.shape)} true labels, {tuple(b.shape)} predictions")
    if ca is None or cb is None:
        import torch
        if a.numel() == 0:
            raise ValueError("no labels")
        top = torch.stack([a.max(), b.max()]).tolist()          # one small read
        ca = top[0] + 1 if ca is None else ca
        cb = top[1] + 1 if cb is None else cb
    return ops.contingency(a, b, int(ca), int(cb)).numpy()


def f1_from_table(table):
    """(macro, micro) F1 from a square count table[true, predicted], as sklearn.metrics.f1_score: macro over the
    labels present in either array, a class without true positives scores 0; micro is the accuracy."""
    t = np.asarray(table, dtype=np.int64)
    if t.ndim != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"table: expected a square matrix, got {t.shape}")
    tp = np.diag(t).astype(np.float64)
    true_n, pred_n = t.sum(axis=1).astype(np.float64), t.sum(axis=0).astype(np.float64)
    present = (true_n + pred_n) > 0
    f1 = 2.0 * tp[present] / (true_n[present] + pred_n[present])
    total = float(t.sum())
    return (float(f1.mean()) if f1.size else 0.0), (float(tp.sum() / total) if total else 0.0)


def nmi_ari_from_table(table):
    """(NMI, ARI) from a count table[true, predicted], as sklearn.metrics: NMI with natural logarithms and the
    arithmetic mean of the entropies (1.0 when both labellings are a single cluster), ARI in its pair-count form."""
    t = np.asarray(table, dtype=np.int64)
    t = t[t.sum(axis=1) > 0][:, t.sum(axis=0) > 0]
    a, b = t.sum(axis=1), t.sum(axis=0)
    n = int(t.sum())
    # NMI
    if a.size <= 1 and b.size <= 1:
        nmi = 1.0
    elif a.size == 1 or b.size == 1:
        nmi = 0.0
    else:
        i, j = np.nonzero(t)
        nij = t[i, j].astype(np.float64)
        outer = a[i].astype(np.int64) * b[j].astype(np.int64)
        log_outer = -np.log(outer) + np.log(a.sum()) + np.log(b.sum())
        terms = (nij / n) * (np.log(nij) - np.log(n)) + (nij / n) * log_outer
        terms = np.where(np.abs(terms) < np.finfo(np.float64).eps, 0.0, terms)
        mi = max(float(terms.sum()), 0.0)
        if abs(mi) < np.finfo(np.float64).eps:
            nmi = 0.0
        else:
            def entropy(c):
                c = c[c > 0].astype(np.float64)
                return -float(np.sum((c / c.sum()) * (np.log(c) - np.log(c.sum()))))
            nmi = float(mi / max(0.5 * (entropy(a) + entropy(b)), np.finfo(np.float64).eps))
    # ARI: exact integer pair counts
    cells = [[int(v) for v in row] for row in t]            # Python integers: no overflow at any n
    ai, bj = [int(v) for v in a], [int(v) for v in b]
    sum_sq = sum(v * v for row in cells for v in row)
    fp = sum(v * bj[j] for row in cells for j, v in enumerate(row)) - sum_sq
    fn = sum(v * ai[i] for i, row in enumerate(cells) for v in row) - sum_sq
    tp = sum_sq - n
    tn = n * n - fp - fn - sum_sq
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        ari = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return nmi, float(ari)


def f1_scores(y_true, y_pred, n_classes=None):
    """(macro, micro) F1 of two label vectors (NumPy or GPU tensors): a contingency table on the GPU, the scores
    from it on the host."""
    return f1_from_table(_table(y_true, y_pred, n_classes, n_classes) if n_classes is not None else
                         _square(_table(y_true, y_pred)))


def _square(t):
    c = max(t.shape)
    out = np.zeros((c, c), dtype=np.int64)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def nmi_ari(y_true, y_pred):
    """(NMI, ARI) of two labellings (NumPy or GPU tensors)."""
    return nmi_ari_from_table(_table(y_true, y_pred))


def _kmeanspp(x, k, rs):
    """k-means++ seeding: k rows of x, the first uniform, each next one drawn with probability proportional to its
    squared distance to the chosen ones.  The k uniform draws come from the host RandomState; the distances, their
    running sum and the search for the drawn row are torch ops on the device (no read-back)."""
    import torch
    n = x.shape[0]
    u = torch.as_tensor(rs.random_sample(k), dtype=torch.float64, device=x.device)
    first = torch.clamp((u[0] * n).long(), max=n - 1)
    centres = [x[first]]
    d2 = ((x - centres[0]) ** 2).sum(dim=1, dtype=torch.float64)
    for j in range(1, k):
        cum = torch.cumsum(d2, 0)
        pick = torch.clamp(torch.searchsorted(cum, (u[j] * cum[-1]).reshape(1), right=True)[0], max=n - 1)
        centres.append(x[pick])
        d2 = torch.minimum(d2, ((x - centres[-1]) ** 2).sum(dim=1, dtype=torch.float64))
    return torch.stack(centres).contiguous()


def _lloyd(x, init, max_iter, tol_abs):
    import torch
    from . import ops
    centres, prev, history = init, None, []
    n_iter, converged = 0, False
    for it in range(1, max_iter + 1):
        step = ops.kmeans_step(x, centres, prev, want_d2=False)
        history.append(step["inertia"])
        shift = ((step["centres"] - centres).double() ** 2).sum().reshape(1)
        changed, shift = torch.cat([step["changed"].double(), shift]).tolist()      # the one small read of the iteration
        n_iter, labels = it, step["labels"]
        if changed == 0:                    # the labels are the assignment to `centres`, which are their means
            converged = True
            break
        prev, centres = labels, step["centres"]
        if tol_abs > 0 and shift <= tol_abs:
            break
    if not converged:                       # the labels of the centres that are returned
        step = ops.kmeans_step(x, centres, None, want_d2=False)
        labels = step["labels"]
        history.append(step["inertia"])
    hist = torch.cat(history).cpu().numpy()
    return dict(labels=labels, centers=centres, inertia=float(hist[-1]), n_iter=n_iter, init_centers=init,
                inertia_history=hist)


def kmeans(x, k, init=None, seed=None, n_init=1, max_iter=300, tol=1e-4, device=None):
    """Lloyd's k-means on the GPU (han_kmeans_step per iteration).  init: an explicit (k, d) array, or None for
    k-means++ seeding with the uniform draws of np.random.RandomState(seed) (a RandomState may be passed as seed).
    Stops when no label changed, when the centres moved by sum |dc|^2 <= tol * mean per-column variance of x (not
    with tol=0), or after max_iter iterations.  Returns dict(labels (n,) int32, centers (k, d), inertia, n_iter,
    init_centers, inertia_history): tensors on the device, the labels being the assignment to the returned centres;
    inertia_history[i] is the inertia of the centres that iteration i + 1 started from.  A cluster that loses all its
    rows keeps its centre (scikit-learn relocates it).  With n_init > 1 the fit of lowest inertia is returned."""
    n, d = _shape2(x, "x")
    if isinstance(k, bool) or int(k) != k or k < 1 or k > KMEANS_MAX_K:
        raise ValueError(f"k = {k!r}: expected an integer in [1, {KMEANS_MAX_K}]")
    if k > n:
        raise ValueError(f"k = {k} clusters of {n} rows")
    if init is not None and tuple(init.shape) != (k, d):
        raise ValueError(f"init: shape {tuple(init.shape)}, expected {(k, d)}")
    if n_init < 1 or max_iter < 1 or tol < 0:
        raise ValueError("n_init >= 1, max_iter >= 1 and tol >= 0 are required")
    dev = _pick_device(device, x)
    x = _embed(x, dev)
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    tol_abs = float(tol) * float(x.var(dim=0, unbiased=False).mean()) if tol > 0 else 0.0
    best = None
    for _ in range(1 if init is not None else int(n_init)):
        start = _embed(init, dev).contiguous() if init is not None else _kmeanspp(x, int(k), rs)
        fit = _lloyd(x, start, int(max_iter), tol_abs)
        if best is None or fit["inertia"] < best["inertia"]:
            best = fit
    return best


SILHOUETTE_MAX_K = 64   # han_silhouette
SILHOUETTE_MAX_D = 512


def _on_host(device, *arrays):
    return device is None and not any(_is_tensor(a) and a.is_cuda for a in arrays)


def _host_array(a, dtype=None):
    return np.asarray(a.numpy() if _is_tensor(a) else a, dtype=dtype)


def _silhouette_device(x, labels, device):
    """(s in the caller's row order, its sum (1,) float64) on the device.  The distinct labels, any integers, become
    codes 0 .. k - 1; a stable sort of the codes groups the rows, one gather of x puts them in that order for
    ops.silhouette, and its rows are scattered back."""
    import torch
    from . import ops
    n, d = _shape2(x, "x")
    dev = _pick_device(device, x, labels)
    lab = labels if _is_tensor(labels) else torch.as_tensor(np.array(labels))
    if lab.dim() != 1 or lab.shape[0] != n:
        raise ValueError(f"labels: shape {tuple(lab.shape)} for {n} rows")
    if lab.is_floating_point() or lab.dtype == torch.bool:
        raise ValueError(f"labels: expected integers, got {lab.dtype}")
    uniq, codes = torch.unique(lab.to(device=dev, dtype=torch.int64), return_inverse=True)
    k = int(uniq.numel())
    if not 2 <= k <= n - 1:                                  # scikit-learn's check_number_of_labels
        raise ValueError(f"Number of labels is {k}. Valid values are 2 to n_samples - 1 (inclusive)")
    if k > SILHOUETTE_MAX_K:
        raise ValueError(f"{k} distinct labels: the device path takes at most {SILHOUETTE_MAX_K}")
    if d > SILHOUETTE_MAX_D:
        raise ValueError(f"x has width {d}: the device path takes at most {SILHOUETTE_MAX_D} columns")
    order = torch.sort(codes, stable=True).indices
    seg = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(codes, minlength=k), 0)
    r = ops.silhouette(_embed(x, dev)[order], seg)
    s = torch.empty_like(r["s"])
    s[order] = r["s"]
    return s, r["sum"]


def _sample(x, labels, sample_size, seed):
    """scikit-learn's sample_size: the rows RandomState(seed).permutation(n)[:sample_size] (seed=None: NumPy's
    global generator, a RandomState: that one)."""
    n = _shape2(x, "x")[0]
    rs = seed if isinstance(seed, np.random.RandomState) else \
        np.random.mtrand._rand if seed is None else np.random.RandomState(seed)
    idx = rs.permutation(n)[:sample_size]

    def pick(a):
        if _is_tensor(a):
            import torch
            return a[torch.as_tensor(idx, device=a.device)]
        return np.asarray(a)[idx]
    return pick(x), pick(labels)


def silhouette_samples(x, labels, device=None):
    """sklearn.metrics.silhouette_samples(x, labels, metric="euclidean"): per row (b - a) / max(a, b), a the mean
    distance to the other rows of its cluster and b the smallest mean distance to another cluster; 0 for a cluster
    of one row.  labels are any integers.  With device=None and no GPU tensor among the arguments: scikit-learn on
    the host in float64, the array it returns.  Otherwise han_silhouette on the device: the (n,) fp32 values in the
    caller's row order, as a tensor on the device.  ValueError unless 2 <= distinct labels <= n - 1; on the device
    also for more than 64 distinct labels or more than 512 columns."""
    if _on_host(device, x, labels):
        from sklearn.metrics import silhouette_samples as sk_samples
        return sk_samples(_host_array(x, np.float64), _host_array(labels), metric="euclidean")
    return _silhouette_device(x, labels, device)[0]


def silhouette_score(x, labels, sample_size=None, seed=None, device=None):
    """sklearn.metrics.silhouette_score(x, labels, metric="euclidean", sample_size=sample_size, random_state=seed)
    (data/exp.py:48): the mean of silhouette_samples, a Python float; with sample_size, over the rows
    RandomState(seed).permutation(n)[:sample_size] only.  Host or device as silhouette_samples; on the device the
    mean is formed from the kernel's float64 sum (one small read)."""
    if _on_host(device, x, labels):
        from sklearn.metrics import silhouette_score as sk_score
        return float(sk_score(_host_array(x, np.float64), _host_array(labels), metric="euclidean", sample_size=sample_size,
                              random_state=seed))
    if sample_size is not None:
        x, labels = _sample(x, labels, sample_size, seed)
    total = _silhouette_device(x, labels, device)[1]
    return float(total) / _shape2(x, "x")[0]


TSNE_MAX_D = 512        # han_tsne_calibrate / han_tsne_step
TSNE_EXPLORATION = 250  # exaggerated iterations (sklearn.manifold.TSNE._EXPLORATION_MAX_ITER)
TSNE_CHECK = 50         # iterations between two reads of the KL divergence and the gradient norm (_N_ITER_CHECK)


def _tsne_init(x, init, seed, dev):
    """The (N, 2) fp32 start on the device.  "random": the numbers scikit-learn draws; "pca": the top two principal
    components (eigh of the D x D covariance in float64), the first with standard deviation 1e-4; else as given."""
    import torch
    n = x.shape[0]
    if isinstance(init, str):
        if init == "random":
            rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
            return torch.as_tensor(np.float32(1e-4) * rs.standard_normal(size=(n, 2)).astype(np.float32)).to(dev)
        if init != "pca":
            raise ValueError(f"init = {init!r}: expected 'pca', 'random' or an (n, 2) array")
        xc = x.to(torch.float64)
        xc = xc - xc.mean(0, keepdim=True)
        vec = torch.linalg.eigh(xc.T @ xc)[1]                # ascending eigenvalues
        if vec.shape[1] < 2:
            vec = torch.cat([torch.zeros_like(vec), vec], 1)
        y = xc @ vec[:, [-1, -2]]
        return (y / y[:, 0].std(unbiased=False) * 1e-4).to(torch.float32).contiguous()
    y = _embed(init, dev)
    if tuple(y.shape) != (n, 2):
        raise ValueError(f"init: shape {tuple(y.shape)}, expected ({n}, 2)")
    return y.clone().contiguous()


def _tsne_device(x, perplexity, early_exaggeration, learning_rate, max_iter, init, seed, n_iter_without_progress,
                 min_grad_norm, device, return_info):
    import torch
    from . import ops
    n, d = _shape2(x, "x")
    if _is_tensor(x) and not x.is_cuda:
        raise ValueError("x: a CPU tensor with device= set; pass a GPU tensor or a NumPy array")
    if not perplexity < n:
        raise ValueError(f"perplexity ({perplexity}) must be less than n_samples ({n})")
    if d > TSNE_MAX_D:
        raise ValueError(f"x has width {d}: the device path takes at most {TSNE_MAX_D} columns")
    dev = _pick_device(device, x)
    x = _embed(x, dev)
    if isinstance(learning_rate, str) and learning_rate != "auto":
        raise ValueError(f"learning_rate = {learning_rate!r}: expected 'auto' or a number")
    lr = max(n / early_exaggeration / 4.0, 50.0) if isinstance(learning_rate, str) else float(learning_rate)
    y = _tsne_init(x, init, seed, dev)
    calib = ops.tsne_calibrate(x, perplexity)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    kl = float("nan")

    def descend(it, end, exaggeration, momentum, patience):
        """_gradient_descent from iteration `it` to `end`: the error and the norm are read every TSNE_CHECK steps"""
        nonlocal kl
        best, best_it = float("inf"), it
        i = it
        for i in range(it, end):
            check = (i + 1) % TSNE_CHECK == 0
            r = ops.tsne_step(x, calib, y, update, gains, exaggeration, momentum, lr, want_kl=check or i == end - 1)
            if check or i == end - 1:
                stats = r["stats"].cpu()                     # the one synchronisation
                kl = float(stats[2])
            if check:
                if kl < best:
                    best, best_it = kl, i
                elif i - best_it > patience:
                    break
                if float(stats[1]) ** 0.5 <= min_grad_norm:
                    break
        return i + 1

    it = descend(0, min(TSNE_EXPLORATION, max_iter), early_exaggeration, 0.5, TSNE_EXPLORATION) if max_iter > 0 else 0
    if it < max_iter:
        update.zero_()
        gains.fill_(1.0)
        it = descend(it, max_iter, 1.0, 0.8, n_iter_without_progress)
    if return_info:
        return y, dict(kl_divergence=kl, n_iter=it, calibration_passes=int(calib["passes"]),
                       open_rows=int(calib["open_rows"].cpu()[0]))
    return y


def tsne(x, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, init="pca", seed=None,
         n_iter_without_progress=300, min_grad_norm=1e-7, device=None, return_info=False):
    """The two-dimensional t-SNE picture of the embeddings (sklearn.manifold, jhyexp.py:16 / data/exp.py:20):
    scikit-learn's TSNE(n_components=2, method="exact", ...).fit_transform(x).
    device=None: that call on the host, the (n, 2) array it returns (init / seed are its init / random_state).
    With a device: han_tsne_calibrate and han_tsne_step, the same schedule -- learning_rate "auto" is
    max(n / early_exaggeration / 4, 50); 250 exaggerated iterations at momentum 0.5, the rest at 0.8; the KL
    divergence and the gradient norm are read every 50 iterations, and the run stops on min_grad_norm or after
    n_iter_without_progress iterations without a better KL -- and the (n, 2) fp32 coordinates stay on the device.
    init: "random" (1e-4 * RandomState(seed).standard_normal((n, 2)).astype(float32), scikit-learn's numbers), "pca" (top two
    principal components, the first with standard deviation 1e-4) or an (n, 2) array / tensor, used as given.
    return_info=True adds dict(kl_divergence, n_iter): the KL divergence at the last iterate the loop evaluated and the
    iterations run (on the host scikit-learn's kl_divergence_ and n_iter_, the index of the last one); on the device also
    calibration_passes and open_rows.  The optimisation is chaotic: host and device runs from one start end in
    different pictures of the same quality.  ValueError for perplexity >= n and, on the device, for more than 512
    columns or a CPU tensor."""
    if device is None:
        from sklearn.manifold import TSNE
        est = TSNE(n_components=2, method="exact", perplexity=perplexity, early_exaggeration=early_exaggeration,
                   learning_rate=learning_rate, max_iter=max_iter, init=init if isinstance(init, str) else _host_array(init, np.float32),
                   random_state=seed, n_iter_without_progress=n_iter_without_progress, min_grad_norm=min_grad_norm)
        y = est.fit_transform(_host_array(x))
        return (y, dict(kl_divergence=float(est.kl_divergence_), n_iter=int(est.n_iter_))) if return_info else y
    return _tsne_device(x, float(perplexity), float(early_exaggeration), learning_rate, int(max_iter), init, seed,
                        n_iter_without_progress, min_grad_norm, device, return_info)


def _my_knn_device(x, y, k, split_list, time, shuffle, seed, verbose, device):
    import torch
    rng = np.random.RandomState(seed) if not isinstance(seed, np.random.RandomState) else seed
    dev = torch.device(device)
    x = _embed(x, dev)
    if x.dim() > 2:
        x = x.squeeze()
    y = _labels(y, dev)
    n_classes = int(y.max()) + 1
    out = {}
    for ss in split_list:
        split = int(x.shape[0] * ss)
        macro, micro = [], []
        for _ in range(time):
            if shuffle:
                perm = torch.as_tensor(rng.permutation(x.shape[0]), device=dev)
                x, y = x[perm], y[perm]
            pred = knn_classify(x[:split], y[:split], x[split:], k, device=dev)
            f = f1_scores(y[split:], pred, n_classes)
            macro.append(f[0])
            micro.append(f[1])
        out[ss] = (float(np.mean(macro)), float(np.mean(micro)))
        if verbose:
            print("KNN({}avg, split:{}, k={}) f1_macro: {:.4f}, f1_micro: {:.4f}".format(
                time, ss, k, out[ss][0], out[ss][1]))
    return out


def _my_kmeans_device(x, y, k, time, seed, verbose, device, silhouette):
    import torch
    dev = torch.device(device)
    x = _embed(x, dev)
    if x.dim() > 2:
        x = x.squeeze()
    y = _labels(y, dev)
    rs = np.random.RandomState(seed) if not isinstance(seed, np.random.RandomState) else seed
    nmi, ari, sil = [], [], []
    for _ in range(time):
        fit = kmeans(x, k, seed=rs, device=dev)
        s = nmi_ari(y, fit["labels"])
        nmi.append(s[0])
        ari.append(s[1])
        if silhouette:
            sil.append(silhouette_score(x, fit["labels"], device=dev))
    return _kmeans_result(nmi, ari, sil, silhouette, verbose)
