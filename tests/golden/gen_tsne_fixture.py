"""Generator of tests/golden/tsne_ref.npz (run by hand from the repository root where scikit-learn is installed;
arrays only in the output).

The reference's evaluation modules import sklearn.manifold (jhyexp.py:16, data/exp.py:20) for the t-SNE picture of
the embeddings.  Exact t-SNE is chaotic -- two runs part after some 50 iterations whatever the precision --, so the
fixture holds POPULATIONS to compare a run with, from eight starts: what scikit-learn's TSNE(method="exact") reaches
and what the float64 restatement tests/tsne_ref.py reaches.  Every KL divergence is evaluated under ONE P, the
float64 joint probabilities of tests/tsne_ref.py.

The fixture holds
  x          (300, 16) fp32: four Gaussian blobs, centres drawn with spread 1.2, unit noise; RandomState(SEED)
  labels     (300,) int64: the blob of every row
  seeds      (8,) int64
  inits      (8, 300, 2) fp32: 1e-4 * RandomState(seed).standard_normal((300, 2)).astype(float32), the product in
             fp32 too: scikit-learn's init="random"
  kl_ref     (8,) float64: KL after 1000 iterations of tsne_ref.tsne from inits[s]
  kl_sk      (8,) float64: KL of TSNE(n_components=2, method="exact", perplexity=30, init=inits[s]).fit_transform(x)
  trust_ref  (8,) float64: sklearn.manifold.trustworthiness(x, y, n_neighbors=5) of the former
  trust_sk   (8,) float64: of the latter
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SEED = 20252
SEEDS = np.arange(8, dtype=np.int64)
PERPLEXITY = 30.0


def blobs():
    rs = np.random.RandomState(SEED)
    labels = rs.permutation(np.repeat(np.arange(4), 75))
    centres = 1.2 * rs.standard_normal((4, 16))
    return (centres[labels] + rs.standard_normal((300, 16))).astype(np.float32), labels.astype(np.int64)


def main():
    from sklearn.manifold import TSNE, trustworthiness
    from tests import tsne_ref as ref
    x, labels = blobs()
    p = ref.joint(ref.d2_rows(x), PERPLEXITY)[0]
    inits = np.stack([np.float32(1e-4) * np.random.RandomState(int(s)).standard_normal(size=(300, 2)).astype(np.float32) for s in SEEDS])
    kl_ref, kl_sk, trust_ref, trust_sk = [], [], [], []
    for s, y0 in zip(SEEDS, inits):
        y = ref.tsne(p, y0)
        y_sk = TSNE(n_components=2, method="exact", perplexity=PERPLEXITY, init=y0).fit_transform(x)
        kl_ref.append(ref.kl_of(p, y))
        kl_sk.append(ref.kl_of(p, y_sk))
        trust_ref.append(trustworthiness(x, y, n_neighbors=5))
        trust_sk.append(trustworthiness(x, y_sk, n_neighbors=5))
        print(int(s), kl_ref[-1], kl_sk[-1], trust_ref[-1], trust_sk[-1], flush=True)
    path = os.path.join(HERE, "tsne_ref.npz")
    np.savez_compressed(path, x=x, labels=labels, seeds=SEEDS, inits=inits, kl_ref=np.array(kl_ref), kl_sk=np.array(kl_sk),
                        trust_ref=np.array(trust_ref), trust_sk=np.array(trust_sk))
    print("tsne_ref.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
