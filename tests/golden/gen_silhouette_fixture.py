"""Generator of tests/golden/exp_silhouette_ref.npz (run by hand in the build container; arrays only in the output).

The reference's second clustering evaluation, ``data/exp.py:25-62``, prints NMI, ARI and the silhouette score of
``time`` k-means fits.  This script imports that module from where the reference lies (``/root/reference/data/exp.py``;
scikit-learn and matplotlib are installed in the build container), runs its own ``my_Kmeans`` after
``np.random.seed(SEED)`` and captures the three numbers from the line it prints, to the 4 decimals it prints.

The fixture holds
  x        (300, 16) fp32: four Gaussian blobs of 75 rows, centres drawn with spread 1.2, unit noise; RandomState(SEED)
  y        (300,) int64: the blob of every row
  seed     SEED
  printed  (3,) float64: NMI, ARI, silhouette as printed by the reference's my_Kmeans(x, y, k=4, time=10)
  labels   (300,) int32: KMeans(n_clusters=4, random_state=RandomState(SEED)).fit(x).labels_
  samples  (300,) float64: sklearn.metrics.silhouette_samples(x as float64, labels, metric="euclidean")
"""
import contextlib
import importlib.util
import io
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20251
REF = "/root/reference/data/exp.py"


def blobs():
    rs = np.random.RandomState(SEED)
    y = np.repeat(np.arange(4), 75)
    centres = 1.2 * rs.standard_normal((4, 16))
    x = (centres[y] + rs.standard_normal((300, 16))).astype(np.float32)
    perm = rs.permutation(300)
    return x[perm], y[perm].astype(np.int64)


def main():
    from sklearn.cluster import KMeans
    from sklearn.metrics import silhouette_samples
    spec = importlib.util.spec_from_file_location("exp_ref", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, y = blobs()
    np.random.seed(SEED)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mod.my_Kmeans(x, y, k=4, time=10)
    line = buf.getvalue().strip().splitlines()[-1]
    printed = [float(v) for v in re.findall(r":\s*(-?\d+\.\d{4})", line)]
    assert len(printed) == 3, line
    labels = KMeans(n_clusters=4, random_state=np.random.RandomState(SEED)).fit(x).labels_.astype(np.int32)
    samples = silhouette_samples(x.astype(np.float64), labels, metric="euclidean")
    assert samples.dtype == np.float64
    path = os.path.join(HERE, "exp_silhouette_ref.npz")
    np.savez_compressed(path, x=x, y=y, seed=np.int64(SEED), printed=np.array(printed, dtype=np.float64),
                        labels=labels, samples=samples)
    print(line)
    print("exp_silhouette_ref.npz:", printed, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
