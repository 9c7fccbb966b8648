"""Test infrastructure for semantic="metapath" (han.pdf eq. 7-9): CPU stand-ins for ops.sem_attn_mean_fwd / _bwd on top
of tests/cpu_backend.py, and the float64 torch oracle of the whole model with tests/sem_metapath_ref.py in place of the
oracle's semantic layer (oracle/ itself is not edited: the pieces are composed here)."""
import numpy as np
import torch

from oracle import han_oracle_torch as ht
from tests import cpu_backend, sem_metapath_ref as ref


def sem_attn_mean_fwd(M, w_omega, b_omega, u_omega, flags=0, out=None, want_mean=False):
    Z, beta, w = ref.forward(*(t.detach().numpy() for t in (M, w_omega, b_omega, u_omega)))
    o = out if out is not None else (None, None)
    res = (cpu_backend._put(o[0], torch.tensor(Z, dtype=torch.float32)),
           cpu_backend._put(o[1], torch.tensor(beta, dtype=torch.float32)))
    return res + (torch.tensor(w),) if want_mean else res


def sem_attn_mean_bwd(M, w_omega, b_omega, u_omega, beta, dZ, out=None, flags=0):
    g = ref.backward(*(t.detach().numpy() for t in (M, w_omega, b_omega, u_omega, dZ)), beta=beta.detach().numpy())
    res = tuple(torch.tensor(x, dtype=torch.float32) for x in g)
    o = out if out is not None else (None,) * 3
    return (res[0],) + tuple(cpu_backend._put(o[i], res[i + 1]) for i in range(3))


def install(monkeypatch):
    """tests/cpu_backend.py plus the two stand-ins above, patched into han_amd.ops for one test."""
    from han_amd import ops
    for n in cpu_backend._NAMES:
        monkeypatch.setattr(ops, n, getattr(cpu_backend, n))
    monkeypatch.setattr(ops, "sem_attn_mean_fwd", sem_attn_mean_fwd)
    monkeypatch.setattr(ops, "sem_attn_mean_bwd", sem_attn_mean_bwd)
    return ops


class RefSemanticMean(torch.autograd.Function):
    """tests/sem_metapath_ref.py as a float64 autograd node: its forward and its closed-form backward."""

    @staticmethod
    def forward(ctx, m, w, b, u):
        ctx.save_for_backward(m, w, b, u)
        Z, beta, _ = ref.forward(*(t.detach().numpy() for t in (m, w, b, u)))
        beta = torch.tensor(beta)
        ctx.mark_non_differentiable(beta)
        return torch.tensor(Z), beta

    @staticmethod
    def backward(ctx, dZ, _dbeta):
        m, w, b, u = ctx.saved_tensors
        return tuple(torch.tensor(g) for g in ref.backward(*(t.detach().numpy() for t in (m, w, b, u)), dZ.numpy()))


def hetegat_forward(x_list, graphs, bp):
    """oracle.han_oracle_torch.hetegat_forward (one node-attention layer, CSR graphs, no dropout) with the published
    semantic attention: logits (N,C), final_embed (N,D), beta (P,)."""
    embeds = [ht.node_attention_csr(x, g[0], g[1], bp["W"][p], bp["a1"][p], bp["b1"][p], bp["a2"][p], bp["b2"][p],
                                    bp["c"][p])[:, None, :] for p, (x, g) in enumerate(zip(x_list, graphs))]
    m = torch.cat(embeds, dim=1)
    final_embed, beta = RefSemanticMean.apply(m, bp["w_omega"], bp["b_omega"], bp["u_omega"])
    hc = bp["Wc"].shape[0]
    logits = sum(final_embed @ bp["Wc"][i] + bp["bc"][i] for i in range(hc)) / hc
    return logits, final_embed, beta


def loss_and_grads(prob, bp):
    """Masked softmax cross-entropy of the problem on the oracle above and its gradient for every parameter."""
    from oracle import han_oracle as ho
    bpo = {k: v.clone().requires_grad_(True) for k, v in bp.items()}
    og = [tuple(torch.tensor(t) for t in ho.bias_to_csr(b)) for b in prob["biases"]]
    logits, embed, beta = hetegat_forward([torch.tensor(prob["x"][0])] * prob["p"], og, bpo)
    loss = ht.masked_softmax_cross_entropy(logits, torch.tensor(prob["onehot"]), torch.tensor(prob["mask"]))
    loss.backward()
    return (float(loss.detach()), logits.detach().numpy(), embed.detach().numpy(), beta.numpy(),
            {k: np.asarray(bpo[k].grad) for k in ht.PARAM_ORDER})
