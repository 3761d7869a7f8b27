"""GPU: the DeBERTa-v2 / v3 path (csrc/deberta.hip, the Disentangled policy of csrc/varlen.h's attention tile,
tensor_truth_amd/deberta.py).

* ``tt_attention_disentangled[_f16]`` against an fp64 softmax attention with both position terms, on the element-rounded operands.
  The bound is tests/test_mpnet_gpu.py's, per output element and derived from the fp64 terms, with the score's error grown by what
  the two position terms add: the tables are fp32 sums of 64 products of 16-bit operands, LAM u sqrt(64) (|Q| . |PK| + |K| . |PQ|),
  and the two fp32 additions and the scaling round 3 u (|q.k| + |C| + |P|) more.  The mirrored index, a dropped position-to-content
  term and that term read from the query's row instead of the key's are defects the bound must catch: shown on the fp64 references
  themselves before the kernel is compared.
* The fixture checkpoint (tests/golden/make_deberta_golden.py) through ``HipSentenceTransformerRerank``: hidden states within
  2 e_<type> of the fp64 model's, e_<type> the same model's own error in that type on the CPU, read from the fixture at test time
  (the factor 2 is the one the ModernBERT, Gemma and MPNet tests give a second 16-bit implementation); logits within 2 x the fixture's
  own 16-bit logit error; clearly ordered pairs keep their order; the score is the logit's sigmoid; every defect reference used for
  the type outside the bound.
* A batch of one 510-token sequence among sixty-three 1-token sequences; one layer at the published base width against transformers
  in fp32 on the device; strings through ``postprocess_nodes``; refused arguments.
Every figure is printed before it is asserted.
"""
import ctypes
import dataclasses
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAME = "deberta_v3_ce"
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
KEY = {"bfloat16": "bf16", "float16": "fp16"}
FACTOR = 2.0
U = 2.0 ** -24
LAM = 4.0
# what the kernel rounds: P and the output to the element type (fp16: subnormals on a grid of 2^-24)
EPS = {torch.bfloat16: dict(p=2.0 ** -8 + 2 * U, p_abs=0.0, out=2.0 ** -8 + 2 * U, out_abs=0.0),
       torch.float16: dict(p=2.0 ** -11 + 2 * U, p_abs=2.0 ** -25, out=2.0 ** -11 + 2 * U, out_abs=2.0 ** -25)}
ATT_LENS = [1, 8, 9, 92, 129, 300]      # packed back to back: 8-row groups shared, 539 rows in 640
ATT_HEADS = 4
SPAN, MAX_POS = 256, 512


def _lib_and_stream(dev):
    from tensor_truth_amd import _lib

    return _lib, _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream


def _sfx(dt):
    return "_f16" if dt == torch.float16 else ""


def _v8(x):                                          # [T][H] -> the V8 layout [T/8][H][8]
    T, H = x.shape
    return x.reshape(T // 8, 8, H).permute(0, 2, 1).contiguous()


def _ratio(err, bound):
    """largest error in units of its bound (an exact result under a zero bound counts as 0)"""
    assert torch.isfinite(bound).all() and (bound >= 0).all(), "the bound itself is not finite"
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


# ---- disentangled attention against fp64 ----------------------------------------------------------------------------------------
def _disentangled_reference(q, k, v, pk, pq, dist_index, starts, lens, heads, eps=None, kind="right"):
    """fp64 attention of (q, k, v) [T][H] per sequence and head, scores (q.k + q.PK[i] + k.PQ[i]) / sqrt(192) with i =
    dist_index[query - key + 511] -> (O, bound) over the sequences' rows in order; bound None without eps.  The defects: "mirrored"
    reads i(key - query), "nop2c" drops k.PQ[i], "p2cq" reads the position-to-content term from the query's row (q's K . PQ[i])."""
    dh, scale = 64, 1.0 / math.sqrt(3 * 64)
    n_pos = pk.shape[0]
    PK, PQ = (x.double().view(n_pos, heads, dh).transpose(0, 1) for x in (pk, pq))          # [h][n_pos][64]
    outs, bounds = [], []
    for s0, n in zip(starts, lens):
        Q, K, V = (x[s0:s0 + n].double().view(n, heads, dh).transpose(0, 1) for x in (q, k, v))
        i = torch.arange(n, device=q.device)
        d = i[:, None] - i[None, :]                                       # query - key
        idx = dist_index.long()[(-d if kind == "mirrored" else d) + MAX_POS - 1]            # [q][k]
        gi, git = idx.expand(heads, n, n), idx.t().expand(heads, n, n)

        def terms(Qm, Km, PKm, PQm):
            c2p = torch.gather(Qm @ PKm.transpose(1, 2), -1, gi)                              # [h][q][k] = Q[q] . PK[i(q, k)]
            if kind == "p2cq":                                                                # K[q] . PQ[i(q, k)]: the query's row
                p2c = torch.gather(Km @ PQm.transpose(1, 2), -1, gi)
            else:                                                                             # [k][q] = K[k] . PQ[i(q, k)], transposed
                p2c = torch.gather(Km @ PQm.transpose(1, 2), -1, git).transpose(1, 2)
            if kind == "nop2c":
                p2c = torch.zeros_like(p2c)
            return Qm @ Km.transpose(1, 2), c2p, p2c

        qk, c2p, p2c = terms(Q, K, PK, PQ)
        S = (qk + c2p + p2c) * scale
        P = torch.softmax(S, dim=-1)
        O = P @ V
        outs.append(O.transpose(0, 1).reshape(n, heads * dh))
        if eps is None:
            continue
        aqk, ac, ap = terms(Q.abs(), K.abs(), PK.abs(), PQ.abs())
        Sa = S.abs()
        dS = (LAM * U * math.sqrt(dh) * (aqk + ac + ap) * scale + 3 * U * (qk.abs() + c2p.abs() + p2c.abs()) * scale
              + 2 * U * (Sa + Sa.amax(-1, keepdim=True)))
        dS = dS * (1.0 + dS.amax())                    # (second order)
        PW, Oa, Vabs = P * dS, O.abs(), V.abs()
        PV = P @ Vabs
        V2 = V.pow(2).sum(1, keepdim=True).sqrt().expand(-1, n, -1)       # sqrt(sum_j v_jd^2) over the sequence's keys
        l_inv = torch.exp(S.amax(-1, keepdim=True) - torch.logsumexp(S, -1, keepdim=True))
        b = (PW @ Vabs + Oa * PW.sum(-1, keepdim=True) + eps["p"] * (PV + Oa) + LAM * eps["p_abs"] * V2 * l_inv
             + LAM * U * math.sqrt(n) * (PV + Oa) + eps["out"] * Oa + eps["out_abs"])
        bounds.append(b.transpose(0, 1).reshape(n, heads * dh))
    return torch.cat(outs), (torch.cat(bounds) if eps is not None else None)


def _attention_inputs(dev, dt, seed=11):
    from tensor_truth_amd.deberta import build_dist_index

    H = ATT_HEADS * 64
    starts = np.concatenate([[0], np.cumsum(ATT_LENS)[:-1]]).tolist()
    T = 640
    assert starts[-1] + ATT_LENS[-1] == 539 and any(s % 8 for s in starts)
    g = torch.Generator(device=dev).manual_seed(seed)
    q, k, v = (torch.randn(T, H, generator=g, device=dev) * s for s in (1.5, 1.5, 1.0))
    pk, pq = (torch.randn(2 * SPAN, H, generator=g, device=dev) for _ in range(2))           # unit scale
    return q.to(dt), k.to(dt), v.to(dt), pk.to(dt).contiguous(), pq.to(dt).contiguous(), build_dist_index(SPAN, MAX_POS).to(dev), starts, T


def _run_disentangled(dev, dt, q, k, v, pk, pq, dist_index, starts, T):
    _lib, lib, st = _lib_and_stream(dev)
    H = ATT_HEADS * 64
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    vt = _v8(v)
    out = torch.zeros(T, H, dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(ATT_LENS, dtype=torch.int32, device=dev)
    need = 2 * ((T * ATT_HEADS * 2 * SPAN * 4 + 255) // 256 * 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    entry = "tt_attention_disentangled" + _sfx(dt)
    rc = getattr(lib, entry)(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(), sl.data_ptr(),
                             len(ATT_LENS), T, ATT_HEADS, 64, max(ATT_LENS), pk.data_ptr(), pq.data_ptr(), 2 * SPAN,
                             dist_index.data_ptr(), MAX_POS, base, need, st)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, ATT_LENS):
        live[s:s + n] = True
    assert (out[~live].view(torch.int16) == 0).all()          # rows of no sequence are not written
    return out, live


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_disentangled_attention_matches_fp64(dev, built_lib, dt):
    q, k, v, pk, pq, dist_index, starts, T = _attention_inputs(dev, dt)
    want, bound = _disentangled_reference(q, k, v, pk, pq, dist_index, starts, ATT_LENS, ATT_HEADS, EPS[dt])
    # teeth first, on the fp64 references themselves: each defect lies more than 2 bounds from the right reference
    others = {}
    for kind in ("mirrored", "nop2c", "p2cq"):
        others[kind], _ = _disentangled_reference(q, k, v, pk, pq, dist_index, starts, ATT_LENS, ATT_HEADS, kind=kind)
        gap = _ratio((others[kind] - want).abs(), bound)
        print(f"\ndisentangled {dt}: the {kind} reference lies {gap:.3g} bounds away")
        assert gap > 2.0, f"the fp64 references of the right form and of '{kind}' are only {gap:.3g} bounds apart on these inputs"
    out, live = _run_disentangled(dev, dt, q, k, v, pk, pq, dist_index, starts, T)
    got = out[live]
    assert torch.isfinite(got.float()).all()
    err = (got.double() - want).abs()
    ratio = _ratio(err, bound)
    print(f"disentangled {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
    assert ratio <= 1.0, f"disentangled {dt}: error {ratio:.3g} x its bound"
    for kind, other in others.items():
        assert _ratio((got.double() - other).abs(), bound) > 1.0, kind


# ---- the fixture checkpoint -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, f"{NAME}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seqs = [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)]
    hidden = {}
    for fn in (f"{NAME}_hidden.npz", f"{NAME}_hidden_510.npz"):
        zh = np.load(os.path.join(GOLDEN, fn))
        hidden.update({int(k.split("_")[1]): zh[k].astype(np.float64) for k in zh.files})
    assert sorted(hidden) == list(range(len(seqs))) and all(hidden[i].shape == (n, 256) for i, n in enumerate(lens))
    defects = {}
    for n in range(3):
        zd = np.load(os.path.join(GOLDEN, f"{NAME}_defects_{n}.npz"))
        defects.update({k: zd[k].astype(np.float64) for k in zd.files})
    return seqs, {k: z[k] for k in z.files}, hidden, defects


@functools.lru_cache(maxsize=None)
def _reranker(dtype, top_n=2):
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank
    from tensor_truth_amd.tokenization import HashTokenizer

    # the fixture directory brings no tokenizer: the test hands token ids (or the hashing stand-in) over, and says so
    return HipSentenceTransformerRerank(model=os.path.join(GOLDEN, NAME), top_n=top_n, device="cuda",
                                        model_kwargs={"torch_dtype": dtype, "tokenizer": HashTokenizer("deberta-v2", 600)})


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_fixture_through_the_reranker(dev, built_lib, dtype):
    from tensor_truth_amd.deberta import DebertaWeights
    from tensor_truth_amd.encoder import pack_tokens

    seqs, z, want, defects = _fixture()
    assert [len(s) for s in seqs] == [1, 9, 17, 92, 130, 300, 510]
    e_ref = float(z[f"e_{KEY[dtype]}"])
    assert 1e-4 < e_ref < 0.5
    bound = FACTOR * e_ref
    rr = _reranker(dtype)
    assert rr.config.arch == "deberta-v2" and rr.config.num_labels == 1 and isinstance(rr.model, DebertaWeights)
    assert rr.activation == "sigmoid" and not rr._use_types and rr.max_length == 512
    batch = pack_tokens(seqs, rr.config)
    assert int(batch.pos[0]) == 0 and batch.max_len == 510
    hidden, _ = rr._encoder.forward_packed(batch)
    torch.cuda.synchronize()
    hidden = hidden.double().cpu().numpy()
    got = [hidden[s:s + n] for s, n in zip(batch.seq_start, batch.seq_len)]
    assert all(np.isfinite(g).all() for g in got)
    err = max(float(np.abs(g - want[i]).max()) for i, g in enumerate(got))
    print(f"\n{NAME} {dtype}: hidden states max |hip - fp64| = {err:.5f}, e_ref = {e_ref:.5f}, ratio = {err / e_ref:.3f}, bound = {bound:.5f}")
    assert err <= bound, f"{NAME} {dtype}: {err:.5f} > {FACTOR} x e_ref = {bound:.5f}"
    # every defect reference used for this type lies outside the bound
    used = [d for d in z["defects"].tolist() if dtype == "float16" or d not in z["defects_fp16_only"].tolist()]
    assert len(used) == (6 if dtype == "float16" else 5) and "linear" in used
    for defect in used:
        gap = max(float(np.abs(got[i] - defects[f"{defect}_{k}"]).max()) for k, i in enumerate(z["defect_idx"].tolist()))
        print(f"{NAME} {dtype}: defect {defect}: max |hip - defect| = {gap:.5f}")
        assert gap > bound, f"the defect reference '{defect}' lands inside the bound"
    # logits: within 2 x the fixture's own 16-bit logit error; clearly ordered pairs keep their order; the score is the sigmoid
    want_logits = z["logits"]
    e_logit = float(np.abs(z[f"logits_{KEY[dtype]}"] - want_logits).max())
    assert 1e-4 < e_logit < 1.0 and np.ptp(want_logits) > 8, "the fixture's own scale"
    scores, logits = rr._encoder.rerank(seqs, max_len=None, want_logits=True)
    scores, logits = scores.double().cpu().numpy(), logits.double().cpu().numpy()
    lerr = float(np.abs(logits - want_logits).max())
    print(f"{NAME} {dtype}: logits max |hip - fp64| = {lerr:.5f}, the model's own = {e_logit:.5f}, ratio = {lerr / e_logit:.3f}")
    assert lerr <= FACTOR * e_logit
    clear = (want_logits[:, None] - want_logits[None, :]) > 4 * e_logit
    assert clear.sum() >= 6 and ((logits[:, None] - logits[None, :])[clear] > 0).all()
    assert np.abs(scores - 1 / (1 + np.exp(-logits))).max() <= 1e-6
    assert np.abs(rr.score_token_pairs(seqs).double().cpu().numpy() - scores).max() == 0


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_long_sequence_among_sixty_three_single_tokens(dev, built_lib, dtype):
    """A batch whose longest sequence (510 tokens) sets the grid and the table width for sixty-three sequences of one token: the
    long sequence's rows are the bits it has in the fixture's own batch, the single tokens identical to each other, every row within
    the bound of the fp64 states."""
    from tensor_truth_amd.encoder import pack_tokens

    seqs, z, want, _ = _fixture()
    bound = FACTOR * float(z[f"e_{KEY[dtype]}"])
    rr = _reranker(dtype)
    enc, cfg = rr._encoder, rr.config
    many = [seqs[0]] * 31 + [seqs[6]] + [seqs[0]] * 32
    batch = pack_tokens(many, cfg)
    assert len(batch.seq_len) == 64 and batch.max_len == 510 and sorted(batch.seq_len.tolist())[:63] == [1] * 63
    hidden, _ = enc.forward_packed(batch)
    ref_batch = pack_tokens(seqs, cfg)
    ref, _ = enc.forward_packed(ref_batch)
    torch.cuda.synchronize()
    s_long, s_ref = int(batch.seq_start[31]), int(ref_batch.seq_start[6])
    assert torch.equal(hidden[s_long:s_long + 510], ref[s_ref:s_ref + 510])
    h = hidden.double().cpu().numpy()
    err_long = float(np.abs(h[s_long:s_long + 510] - want[6]).max())
    ones = np.stack([h[int(s)] for i, s in enumerate(batch.seq_start) if i != 31])
    err_one = float(np.abs(ones - want[0][0]).max())
    print(f"\n{dtype}: 510-token sequence max error {err_long:.5f}, single tokens {err_one:.5f}, bound {bound:.5f}")
    assert (ones == ones[0]).all() and err_long <= bound and err_one <= bound
    scores = enc.rerank_packed(batch)
    assert torch.isfinite(scores).all() and (scores[:31] == scores[0]).all() and (scores[32:] == scores[0]).all()


# ---- one layer at the published width -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_layer_at_the_published_base_width(dev, built_lib, dtype):
    """768 wide, 12 heads, FFN 3072, seeded weights, 238 token rows padded to 256: against transformers' DebertaV2Model in fp32 on the
    device, within 2 x the deviation of transformers' own run in the 16-bit type there."""
    from transformers import DebertaV2Config, DebertaV2Model

    from tensor_truth_amd.deberta import MXBAI_RERANK_BASE, DebertaWeights, synthetic_state
    from tensor_truth_amd.encoder import Encoder, pack_tokens

    dt = DTYPES[dtype]
    cfg = dataclasses.replace(MXBAI_RERANK_BASE, vocab_size=1000, layers=1)
    state = synthetic_state(cfg, seed=7)
    hf = DebertaV2Model(DebertaV2Config(
        vocab_size=cfg.vocab_size, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=1,
        max_position_embeddings=512, relative_attention=True, position_buckets=256, max_relative_positions=-1, share_att_key=True,
        pos_att_type=["p2c", "c2p"], norm_rel_ebd="layer_norm", position_biased_input=False, type_vocab_size=0,
        layer_norm_eps=cfg.ln_eps, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pad_token_id=0)).eval()
    body = {k: v for k, v in state.items() if not k.startswith(("pooler.", "classifier."))}
    missing, unexpected = hf.load_state_dict(body, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    g = np.random.default_rng(5)
    seqs = [[1] + g.integers(4, cfg.vocab_size, n - 2).tolist() + [2] for n in (200, 37)] + [[1]]
    batch = pack_tokens(seqs, cfg)
    assert batch.n_rows == 256 and batch.n_tokens == 238
    enc = Encoder(DebertaWeights(cfg, state, dev, dtype=dt))
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()

    def run(model):
        with torch.no_grad():
            return [model(input_ids=torch.tensor([s], device=dev)).last_hidden_state[0].double() for s in seqs]

    want = run(hf.to(dev, torch.float32))
    low = run(hf.to(dt))
    e_ref = max(float((a - b).abs().max()) for a, b in zip(low, want))
    err = max(float((hidden[s:s + n].double() - w).abs().max()) for s, n, w in zip(batch.seq_start, batch.seq_len, want))
    print(f"\nbase width {dtype}: max |hip - fp32| = {err:.5f}, transformers' own {dtype} error = {e_ref:.5f}, ratio = {err / e_ref:.3f}")
    assert 1e-4 < e_ref < 0.5 and err <= FACTOR * e_ref


# ---- surface -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_strings_in_nodes_out(dev, built_lib, dtype):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.schema import NodeWithScore, QueryBundle, TextNode
    from tensor_truth_amd.tokenization import HashTokenizer

    rr = _reranker(dtype, top_n=3)
    query = "which passage is about attention"
    passages = [f"passage number {i} " + " ".join(f"word{(7 * i + j) % 50}" for j in range(5 + 9 * i)) for i in range(6)]
    per_passage = rr.predict([(query, p) for p in passages])
    assert len(per_passage) == 6 and all(0.0 < s < 1.0 for s in per_passage) and len(set(per_passage)) == 6
    nodes = [NodeWithScore(node=TextNode(text=p, id_=f"p{i}"), score=0.25) for i, p in enumerate(passages)]
    ranked = rr.postprocess_nodes(nodes, query_bundle=QueryBundle(query_str=query))
    order = sorted(range(6), key=lambda i: -per_passage[i])[:3]
    assert [n.node.id_ for n in ranked] == [f"p{i}" for i in order] and [n.score for n in ranked] == [per_passage[i] for i in order]
    assert rr.predict([]) == [] and not rr.accepts_token_source("hash:deberta-v2:600")
    ids, _ = rr._tokenizer.encode_pair(query, passages[0], rr.max_length)
    assert ids[0] == 1 and ids[-1] == 2 and ids.count(2) == 2
    # a DeBERTa directory handed to the embedder is refused: cross-encoders only
    with pytest.raises(NotImplementedError, match="out of scope"):
        HipHuggingFaceEmbedding(os.path.join(GOLDEN, NAME), device="cuda",
                                model_kwargs={"torch_dtype": dtype, "tokenizer": HashTokenizer("deberta-v2", 600)})


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_bad_arguments_refused_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd.deberta import _DbW
    from tensor_truth_amd.encoder import _EncW, _LayerW

    _, lib, st = _lib_and_stream(dev)
    fwd, wsb, att, head = (getattr(lib, n + sfx) for n in ("tt_deberta_forward", "tt_deberta_workspace_bytes",
                                                            "tt_attention_disentangled", "tt_deberta_head"))
    layers = (_LayerW * 1)()
    ptrs = (ctypes.c_void_p * 1)(1)

    def weights(pos_key=True, dist_index=1, n_pos=512, max_pos=512, **kw):
        a = dict(hidden=768, layers=1, heads=12, ffn=3072, vocab=1000, max_pos=512, type_vocab=1, ln_eps=1e-7, word_emb=1, emb_ln_g=1,
                 emb_ln_b=1)
        a.update(kw)
        pp = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        return _DbW(enc=_EncW(layer=ctypes.cast(layers, ctypes.POINTER(_LayerW)), **a), pos_key=pp if pos_key else None, pos_query=pp,
                    dist_index=dist_index, n_pos=n_pos, max_pos=max_pos)

    def err():
        return lib.tt_last_error().decode()

    def refused(w, rc_want, text):
        assert wsb(ctypes.byref(w), 256) == 0
        rc = fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc == rc_want and text in err(), (rc, err())

    base_ws = wsb(ctypes.byref(weights()), 256)
    assert base_ws > 2 * 256 * 12 * 512 * 4                                      # the two score tables are in it
    for kw, text in ((dict(hidden=1152, heads=18), "hidden"), (dict(hidden=320, heads=5), "hidden"), (dict(heads=8), "head_dim"),
                     (dict(hidden=384, heads=12), "head_dim"), (dict(ffn=1100), "ffn"), (dict(n_pos=0), "n_pos"),
                     (dict(n_pos=510), "n_pos"), (dict(max_pos=1024), "max_pos"), (dict(max_pos=0), "max_pos")):
        refused(weights(**kw), -2, text)
    layers[0].qkv_w8 = 1                                   # an fp8 pointer in a layer
    refused(weights(), -2, "qkv_w8")
    layers[0].qkv_w8 = None
    refused(weights(pos_key=False), -1, "pos_key")
    refused(weights(dist_index=None), -1, "dist_index")
    ptrs[0] = None
    refused(weights(), -1, "pos_key")
    ptrs[0] = 1
    # tables that do not fit in size_t
    big = weights(n_pos=1 << 30)
    assert wsb(ctypes.byref(big), (1 << 31) - 128) == 0
    w = weights(layers=0)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    need = wsb(ctypes.byref(w), 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = fwd(ctypes.byref(w), p, p, p, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "type_ids" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 0, 256, 16, p, base, need, st)
    assert rc == -1 and "n_seq" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 200, 16, p, base, need, st)
    assert rc == -1 and "n_rows" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need - 1, st)
    assert rc != 0 and "workspace" in err()
    w1k = weights(layers=0)
    need1k = wsb(ctypes.byref(w1k), 1024)
    ws1k = torch.empty(need1k + 256, dtype=torch.uint8, device=dev)
    rc = fwd(ctypes.byref(w1k), p, p, None, p, p, 1, 1024, 600, p, (ws1k.data_ptr() + 255) // 256 * 256, need1k, st)
    assert rc == -1 and "max_len" in err()                 # a sequence longer than max_pos
    # the head: no head tensors, a pooling other than the first token
    sc = torch.zeros(4, device=dev)
    assert head(ctypes.byref(w), p, 768, p, p, 4, 0, sc.data_ptr(), None, st) == -1 and "classification head" in err()
    assert head(ctypes.byref(w), p, 768, p, p, 4, 1, sc.data_ptr(), None, st) == -1 and "pooling" in err()
    # the building block
    tb = 2 * 256 * 4 * 512 * 4
    wsa = torch.empty(tb + 256, dtype=torch.uint8, device=dev)
    ba = (wsa.data_ptr() + 255) // 256 * 256

    def attention(head_dim=64, k_col0=256, max_len=16, pos_key=p, n_pos=512, dist=p, max_pos=512, ws_ptr=ba, ws_bytes=tb):
        return att(p, 768, 0, k_col0, p, 2048, p, 256, p, p, 1, 256, 4, head_dim, max_len, pos_key, p, n_pos, dist, max_pos, ws_ptr,
                   ws_bytes, st)

    assert attention(head_dim=32) == -2 and "head_dim" in err()
    assert attention(pos_key=None) == -1 and "null" in err()
    assert attention(dist=None) == -1 and "null" in err()
    assert attention(k_col0=600) == -1                     # K columns past the row
    assert attention(max_len=300) == -1                    # max_len > n_rows
    assert attention(n_pos=510) == -2 and "n_pos" in err()
    assert attention(max_pos=1024) == -2 and "max_pos" in err()
    assert attention(max_pos=8) == -1 and "max_len" in err()
    assert attention(n_pos=1 << 30) != 0 and ("size_t" in err() or "workspace" in err())
    assert attention(ws_bytes=tb - 1) != 0 and "workspace" in err()
    assert attention(ws_ptr=None) != 0 and "workspace" in err()
    torch.cuda.synchronize()
