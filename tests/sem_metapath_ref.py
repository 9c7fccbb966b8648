"""float64 reference of the semantic attention with one weight per meta-path (han_amd/csrc/sem_attn_mean.hip; han.pdf
sec. 4.2, eq. 7-9) and of its closed-form backward (test infrastructure, NumPy only).

    s_ip = u . tanh(W^T M_ip + b)      w_p = (1/N) sum_i s_ip      beta = softmax_p(w)      Z_i = sum_p beta_p M_ip

    dbeta_p = sum_i <dZ_i, M_ip>       dw_p = beta_p (dbeta_p - sum_q beta_q dbeta_q)       ds_ip = dw_p / N
    dpre_ip = ds_ip u (1 - v_ip^2)     dM_ip = beta_p dZ_i + W dpre_ip
    dW = sum_ip M_ip (x) dpre_ip       db = sum_ip dpre_ip         du = sum_ip ds_ip v_ip

tests/test_sem_metapath_host.py checks the backward against float64 autograd of the forward.
"""
import numpy as np


def up(*xs):
    return tuple(np.asarray(x, dtype=np.float64) for x in xs)


def forward(M, W, b, u):
    """M (N,P,D), W (D,A), b (A,), u (A,) -> Z (N,D), beta (P,), w (P,) in float64."""
    M, W, b, u = up(M, W, b, u)
    v = np.tanh(M @ W + b)                 # (N,P,A)
    w = (v @ u).mean(axis=0)               # (P,)
    e = np.exp(w - w.max())
    beta = e / e.sum()
    Z = np.einsum("p,npd->nd", beta, M)
    return Z, beta, w


def backward(M, W, b, u, dZ, beta=None):
    """dM (N,P,D), dW (D,A), db (A,), du (A,) in float64.  beta: the weights the backward kernel is given (the fp32
    output of the GPU forward), so that the forward's error is not charged twice; None: the reference's own."""
    M, W, b, u, dZ = up(M, W, b, u, dZ)
    N = M.shape[0]
    beta = forward(M, W, b, u)[1] if beta is None else up(beta)[0]
    v = np.tanh(M @ W + b)
    dbeta = np.einsum("nd,npd->p", dZ, M)
    dw = beta * (dbeta - (beta * dbeta).sum())
    ds = dw / N                                                 # (P,), the same for every node
    dpre = ds[None, :, None] * u[None, None, :] * (1.0 - v * v)  # (N,P,A)
    dM = beta[None, :, None] * dZ[:, None, :] + dpre @ W.T
    dW = np.einsum("npd,npa->da", M, dpre)
    db = dpre.sum(axis=(0, 1))
    du = np.einsum("p,npa->a", ds, v)
    return dM, dW, db, du


def inputs(N, P, D, A, seed, u_scale=1.0):
    """Seeded fp32 inputs: M and dZ standard normal, the parameters with the model's N(0, 0.1^2) (utils/layers.py:145-147),
    u_omega times u_scale (10: beta far from uniform)."""
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s, dtype=np.float32)
    return (f(N, P, D), 0.1 * f(D, A), 0.1 * f(A), np.float32(0.1 * u_scale) * f(A), f(N, D))
