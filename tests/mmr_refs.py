"""References for the MMR tests (tt_mmr_select, include/tt_hip.h): the pairwise similarities in fp64 with their bound, and the
greedy selection restated in ``numpy.float32`` -- every product and difference one rounding, as the kernel's, so the replay is exact."""
import numpy as np
import torch

PENALTIES = {"max": 0, "last": 1}


def gram_fp64(C: torch.Tensor, cand):
    """C: the corpus, [N, D] bf16 (any device); cand: list positions -> corpus rows, entries < 0 or >= N are padding.
    -> (G64 [P, P], bound [P, P], valid [P]) as numpy: the exact dot products of the bf16 rows in fp64 and, per pair,
    ``D * 2^-23 * sum_d |c_i[d] * c_j[d]|``: twice the standard bound gamma_D ~ D * 2^-24 of an fp32 accumulation over D exact
    products (a bf16 x bf16 product has 16 significant bits: exact in fp32); the factor 2 covers whatever order the MFMA adds
    its 32 products in.  Padding positions hold zeros (and a zero bound)."""
    cand = np.asarray(cand, dtype=np.int64)
    n, d = C.shape
    valid = (cand >= 0) & (cand < n)
    rows = torch.as_tensor(np.where(valid, cand, 0), device=C.device)
    X = C.index_select(0, rows).to(torch.float64)
    X = X * torch.as_tensor(valid, device=C.device).to(torch.float64)[:, None]
    g = (X @ X.T).cpu().numpy()
    b = (X.abs() @ X.abs().T).cpu().numpy() * (d * 2.0 ** -23)
    return g, b, valid


def greedy_f32(rel, G, k, lam, penalty, valid=None):
    """The selection rule of tt_mmr_select for ONE query in numpy.float32.  rel [P] fp32, G [P, P] fp32 (G[p][d] is read after the
    pick p), ``penalty`` 0 / "max" or 1 / "last", ``valid`` [P] bool (default: all) -> (mmr [k] fp32, rel [k] fp32, pos [k] int32),
    padded with (-inf, -inf, -1) once nothing can be picked."""
    penalty = PENALTIES.get(penalty, penalty)
    assert penalty in (0, 1)
    rel = np.asarray(rel, dtype=np.float32)
    G = np.asarray(G, dtype=np.float32)
    p_n = rel.shape[0]
    is_open = np.ones(p_n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).copy()
    lam32 = np.float32(lam)
    oml = np.float32(1.0) - lam32
    lr = lam32 * rel                                              # one rounding each
    pen = np.zeros(p_n, dtype=np.float32)
    out_v = np.full(k, -np.inf, dtype=np.float32)
    out_r = np.full(k, -np.inf, dtype=np.float32)
    out_p = np.full(k, -1, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k):
            v = lr if s == 0 else lr - (oml * pen)                # the product is rounded, then the difference
            live = np.flatnonzero(is_open & ~np.isnan(v))
            if live.size == 0:
                break
            # argmax = the FIRST of the largest values: the walk over positions upward with a strict > (so -0 == +0 is a tie)
            best = int(live[np.argmax(v[live])])
            out_v[s], out_r[s], out_p[s] = v[best], rel[best], best
            is_open[best] = False
            g = G[best]
            pen = g.copy() if (penalty == 1 or s == 0) else np.fmax(pen, g)     # fmaxf: a NaN operand loses
    return out_v, out_r, out_p


def bf16_round(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def constructed_rows(dim=128):
    """Four unit rows rounded to bf16 and the query e0: a ~ e0+e1, a' ~ e0+e1+0.05 e2 (a near-duplicate whose score ties a's
    exactly after the rounding), b ~ e0+1.1 e3, f ~ 0.3 e0+e5.  -> (rows [4, dim] fp32 holding bf16 values, query [dim] fp32)."""
    r = np.zeros((4, dim), dtype=np.float64)
    r[0, [0, 1]] = 1.0
    r[1, [0, 1]] = 1.0
    r[1, 2] = 0.05
    r[2, 0], r[2, 3] = 1.0, 1.1
    r[3, 0], r[3, 5] = 0.3, 1.0
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    q = np.zeros(dim, dtype=np.float32)
    q[0] = 1.0
    return bf16_round(r), q
