"""GPU: the NomicBERT / Jina-embeddings-v3 path (csrc/ropebert.hip, tensor_truth_amd/ropebert.py).

* The two fixture checkpoints (tests/golden/make_ropebert_golden.py) through ``HipHuggingFaceEmbedding`` in bf16 and fp16: hidden
  states within 2 e_<type> of the fp64 model's for every length (1 ... 700 tokens), e_<type> the transformers model's own error in
  that type on the CPU, read from the fixture (the factor 2 is the one the ModernBERT, Gemma, MPNet and DeBERTa tests give a second
  16-bit implementation); every defect reference of the fixture used for the type outside that bound; pooled embeddings with
  cos >= 0.999 against fp64.
* The original-layout NomicBERT directory gives the bits of the transformers-layout one.
* The 700-token sequence among sixty-three 1-token sequences: row for row the bits it has alone.
* One layer at each published width (768 / 12 heads / 3072 SwiGLU without biases; 1024 / 16 heads / 4096 GELU with biases), three
  ragged sequences (5, 64, 129 tokens), against a torch fp64 evaluation of the same layer written here, bounded by 2 x the deviation
  of the same evaluation run on the CPU in the 16-bit type.
* Prompts of config_sentence_transformers.json, and arguments refused before a launch.
Every figure is printed before it is asserted.
"""
import ctypes
import dataclasses
import functools
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
KEY = {"bfloat16": "bf16", "float16": "fp16"}
KINDS = {"nomic": "nomic_bert", "jina": "jina_embeddings_v3"}
LENGTHS = [1, 9, 17, 92, 130, 300, 700]
FACTOR = 2.0


@functools.lru_cache(maxsize=None)
def _fixture(kind):
    name = f"ropebert_{kind}"
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seqs = [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)]
    hidden = {}
    for fn in (f"{name}_hidden.npz", f"{name}_hidden_700.npz"):
        zh = np.load(os.path.join(GOLDEN, fn))
        hidden.update({int(k.split("_")[1]): zh[k].astype(np.float64) for k in zh.files})
    assert sorted(hidden) == list(range(len(seqs))) and all(hidden[i].shape == (n, 256) for i, n in enumerate(lens))
    defects = {}
    for dn in z["defects"].tolist():
        zd = np.load(os.path.join(GOLDEN, f"{name}_defect_{dn}.npz"))
        defects[dn] = [zd[f"{dn}_{k}"].astype(np.float64) for k in range(len(z["defect_idx"]))]
    return seqs, {k: z[k] for k in z.files}, hidden, defects


def _embedder(directory, dtype, **kw):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.tokenization import HashTokenizer

    # the fixture directories bring no tokenizer: the tests hand token ids over, and say so
    return HipHuggingFaceEmbedding(directory, device="cuda",
                                   model_kwargs={"torch_dtype": dtype, "tokenizer": HashTokenizer("xlmr", 600)}, **kw)


def _hidden_of(emb, seqs):
    from tensor_truth_amd.encoder import pack_tokens

    batch = pack_tokens(seqs, emb.config)
    hidden, _ = emb._encoder.forward_packed(batch)
    torch.cuda.synchronize()
    return batch, hidden


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_fixture_through_the_embedder(dev, built_lib, kind, dtype):
    from tensor_truth_amd.ropebert import RopeBertWeights

    seqs, z, want, defects = _fixture(kind)
    assert [len(s) for s in seqs] == LENGTHS
    e_ref = float(z[f"e_{KEY[dtype]}"])
    assert 1e-4 < e_ref < 0.5
    bound = FACTOR * e_ref
    emb = _embedder(os.path.join(GOLDEN, f"ropebert_{kind}"), dtype)
    assert emb.config.arch == KINDS[kind] and emb.pooling == "mean" and isinstance(emb._model, RopeBertWeights)
    assert emb.max_length == 2048 and (emb.query_instruction, emb.text_instruction) == ("", "")
    batch, hidden = _hidden_of(emb, seqs)
    assert int(batch.pos[0]) == 0 and batch.max_len == 700 and batch.types is None
    hidden = hidden.double().cpu().numpy()
    got = [hidden[s:s + n] for s, n in zip(batch.seq_start, batch.seq_len)]
    assert all(np.isfinite(g).all() for g in got)
    errs = [float(np.abs(g - want[i]).max()) for i, g in enumerate(got)]
    print(f"\nropebert_{kind} {dtype}: hidden states max |hip - fp64| per length {dict(zip(LENGTHS, np.round(errs, 5)))}, "
          f"e_ref = {e_ref:.5f}, ratio = {max(errs) / e_ref:.3f}, bound = {bound:.5f}")
    assert max(errs) <= bound, f"ropebert_{kind} {dtype}: {max(errs):.5f} > {FACTOR} x e_ref = {bound:.5f}"
    vec = emb.embed_token_batches(seqs).double().cpu().numpy()
    cos = (vec * z["emb"]).sum(1) / np.linalg.norm(vec, axis=1)
    print(f"ropebert_{kind} {dtype}: min cos to the fp64 pooled embeddings = {cos.min():.6f}")
    assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() < 1e-3 and cos.min() >= 0.999
    # every defect reference used for this type lies outside the bound
    used = [d for d in z["defects"].tolist() if dtype == "float16" or d not in z["defects_fp16_only"].tolist()]
    assert set(used) >= {"norope", "interleaved", "theta", "notype", "prenorm", "swapglu" if kind == "nomic" else "nobias"}
    for defect in used:
        gap = max(float(np.abs(got[i] - defects[defect][k]).max()) for k, i in enumerate(z["defect_idx"].tolist()))
        print(f"ropebert_{kind} {dtype}: defect {defect}: max |hip - defect| = {gap:.5f}")
        assert gap > bound, f"the defect reference '{defect}' lands inside the bound"
    # strings go through the tokenizer the caller handed over
    v = np.asarray(emb.get_text_embedding("a few words of text"))
    assert v.shape == (256,) and np.isfinite(v).all() and abs(np.linalg.norm(v) - 1) < 1e-3


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_original_layout_gives_the_same_bits(dev, built_lib, dtype):
    seqs, _, _, _ = _fixture("nomic")
    a = _embedder(os.path.join(GOLDEN, "ropebert_nomic"), dtype)
    b = _embedder(os.path.join(GOLDEN, "ropebert_nomic_orig"), dtype)
    assert b.config == a.config
    _, ha = _hidden_of(a, seqs)
    _, hb = _hidden_of(b, seqs)
    assert torch.isfinite(ha.float()).all() and torch.equal(ha, hb)
    assert torch.equal(a.embed_token_batches(seqs), b.embed_token_batches(seqs))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_long_sequence_among_sixty_three_single_tokens(dev, built_lib, kind, dtype):
    """A batch whose longest sequence (700 tokens) sets the grid for sixty-three sequences of one token: the long sequence's rows
    are the bits it has alone, every row within the bound of the fp64 states."""
    from tensor_truth_amd.encoder import pack_tokens

    seqs, z, want, _ = _fixture(kind)
    bound = FACTOR * float(z[f"e_{KEY[dtype]}"])
    emb = _embedder(os.path.join(GOLDEN, f"ropebert_{kind}"), dtype)
    enc, cfg = emb._encoder, emb.config
    many = [seqs[0]] * 31 + [seqs[6]] + [seqs[0]] * 32
    batch = pack_tokens(many, cfg)
    assert len(batch.seq_len) == 64 and batch.max_len == 700 and sorted(batch.seq_len.tolist())[:63] == [1] * 63
    hidden, _ = enc.forward_packed(batch)
    alone, _ = enc.forward_packed(pack_tokens([seqs[6]], cfg))
    torch.cuda.synchronize()
    s_long = int(batch.seq_start[31])
    assert torch.equal(hidden[s_long:s_long + 700], alone[:700])
    h = hidden.double().cpu().numpy()
    err_long = float(np.abs(h[s_long:s_long + 700] - want[6]).max())
    ones = np.stack([h[int(s)] for i, s in enumerate(batch.seq_start) if i != 31])
    err_one = float(np.abs(ones - want[0][0]).max())
    print(f"\n{kind} {dtype}: 700-token sequence max error {err_long:.5f}, single tokens {err_one:.5f}, bound {bound:.5f}")
    assert (ones == ones[0]).all() and err_long <= bound and err_one <= bound
    vec, _ = enc.embed_packed(batch, pooling="mean")
    cls, _ = enc.embed_packed(batch, pooling="cls")
    assert torch.isfinite(vec).all() and torch.allclose(vec[0], cls[0], atol=1e-6)        # one token: its mean is its first row


# ---- one layer at each published width ---------------------------------------------------------------------------------------------
def _layer_reference(cfg, state, ids, dt):
    """One layer of ``cfg`` on the CPU in ``dt`` (weights and activations; cos / sin from fp32 angles, as the rotary module computes
    them): LayerNorm(word + type[0]) -> post-LN attention with rotate-half RoPE -> post-LN MLP.  -> [n][H] in fp64."""
    F = torch.nn.functional
    sd = {k: v.to(dt) for k, v in state.items()}
    n, H, nh = len(ids), cfg.hidden, cfg.heads
    lin = lambda x, name: F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))  # noqa: E731
    ln = lambda x, name: F.layer_norm(x, (H,), sd[name + ".weight"], sd[name + ".bias"], cfg.ln_eps)  # noqa: E731
    x = sd["embeddings.word_embeddings.weight"][torch.tensor(ids)] + sd["embeddings.token_type_embeddings.weight"][0]
    x = ln(x, "embeddings.LayerNorm")
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64))
    ang = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = (torch.cat([t, t], -1).to(dt)[:, None, :] for t in (ang.cos(), ang.sin()))
    rot = lambda t: torch.cat([-t[..., 32:], t[..., :32]], -1)  # noqa: E731
    p = "layers.0."
    q, k, v = (lin(x, p + f"self_attn.{m}_proj").view(n, nh, 64) for m in "qkv")
    q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
    s = torch.einsum("qhd,khd->hqk", q, k) * (1.0 / math.sqrt(64))
    a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, H)
    x = ln(x + lin(a, p + "self_attn.o_proj"), p + "post_attention_layernorm")
    if cfg.mlp == "swiglu":
        m = lin(F.silu(lin(x, p + "mlp.gate_proj")) * lin(x, p + "mlp.up_proj"), p + "mlp.down_proj")
    else:
        m = lin(F.gelu(lin(x, p + "mlp.fc1")), p + "mlp.fc2")
    return ln(x + m, p + "post_mlp_layernorm").double()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_layer_at_the_published_width(dev, built_lib, kind, dtype):
    from tensor_truth_amd.encoder import Encoder, pack_tokens
    from tensor_truth_amd.ropebert import JINA_V3, NOMIC_BASE, RopeBertWeights, synthetic_state

    dt = DTYPES[dtype]
    cfg = dataclasses.replace(NOMIC_BASE if kind == "nomic" else JINA_V3, vocab_size=1000, layers=1)
    assert (cfg.hidden, cfg.heads, cfg.ffn, cfg.mlp) == ((768, 12, 3072, "swiglu") if kind == "nomic" else (1024, 16, 4096, "gelu"))
    state = synthetic_state(cfg, seed=7)
    g = torch.Generator().manual_seed(8)
    for k in state:                               # sharper attention than N(0, 0.02) gives, so that RoPE is visible
        if "q_proj.weight" in k or "k_proj.weight" in k:
            state[k] = state[k] * 4.0
        elif cfg.biases and k.endswith("proj.bias"):
            state[k] = torch.randn(state[k].shape, generator=g) * 0.2
    rng = np.random.default_rng(5)
    seqs = [rng.integers(4, cfg.vocab_size, n).tolist() for n in (5, 64, 129)]
    batch = pack_tokens(seqs, cfg)
    assert batch.n_rows == 256 and batch.n_tokens == 198 and batch.seq_start.tolist() == [0, 8, 72]
    enc = Encoder(RopeBertWeights(cfg, state, dev, dtype=dt))
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()
    # the weights the device holds are the state rounded to dt: both references start from those
    rounded = {k: v.to(dt).float() for k, v in state.items()}
    want = [_layer_reference(cfg, rounded, s, torch.float64) for s in seqs]
    low = [_layer_reference(cfg, rounded, s, dt) for s in seqs]
    e_ref = max(float((a - b).abs().max()) for a, b in zip(low, want))
    got = [hidden[s:s + n].double().cpu() for s, n in zip(batch.seq_start, batch.seq_len)]
    err = max(float((a - b).abs().max()) for a, b in zip(got, want))
    print(f"\n{kind} width {cfg.hidden} {dtype}: max |hip - fp64| = {err:.5f}, torch's own {dtype} error on the CPU = {e_ref:.5f}, "
          f"ratio = {err / e_ref:.3f}")
    assert all(torch.isfinite(a).all() for a in got) and 1e-4 < e_ref < 0.5 and err <= FACTOR * e_ref
    # the reference has teeth: without RoPE it is further away than the bound
    nr = dataclasses.replace(cfg, rope_theta=1e30)       # every angle but the first pair's vanishes
    far = max(float((_layer_reference(nr, rounded, s, torch.float64) - w).abs().max()) for s, w in zip(seqs, want))
    print(f"{kind} width {cfg.hidden}: a layer with (almost) no rotation lies {far:.5f} away")
    assert far > 2 * FACTOR * e_ref


# ---- prompts ---------------------------------------------------------------------------------------------------------------------------
def test_prompts_of_the_checkpoint_directory(dev, built_lib, tmp_path):
    src = os.path.join(GOLDEN, "ropebert_nomic")
    d = str(tmp_path / "nomic")
    shutil.copytree(src, d)
    with open(os.path.join(d, "config_sentence_transformers.json"), "w") as f:
        json.dump({"prompts": {"query": "search_query: ", "document": "search_document: "}, "default_prompt_name": None}, f)
    emb = _embedder(d, "bfloat16")
    assert (emb.query_instruction, emb.text_instruction) == ("search_query: ", "search_document: ")
    plain = _embedder(src, "bfloat16")
    q = np.asarray(emb.get_query_embedding("what is a tile"))
    assert np.array_equal(q, np.asarray(plain.get_text_embedding("search_query: what is a tile")))
    assert not np.array_equal(q, np.asarray(plain.get_query_embedding("what is a tile")))
    assert np.array_equal(np.asarray(emb.get_text_embedding("a tile")), np.asarray(plain.get_text_embedding("search_document: a tile")))
    # explicit instruction arguments win
    own = _embedder(d, "bfloat16", query_instruction="q: ", text_instruction="")
    assert (own.query_instruction, own.text_instruction) == ("q: ", "")


def test_the_reranker_refuses_these_types(dev, built_lib):
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    for kind, mt in KINDS.items():
        with pytest.raises(ValueError, match=f"{mt} checkpoints are served as embedders only"):
            HipSentenceTransformerRerank(model=os.path.join(GOLDEN, f"ropebert_{kind}"), device="cuda",
                                         model_kwargs={"torch_dtype": "bfloat16"})


@pytest.mark.default_precision
def test_a_dtype_must_be_named(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.tokenization import HashTokenizer

    with pytest.raises(NotImplementedError, match="bfloat16.*float16"):
        HipHuggingFaceEmbedding(os.path.join(GOLDEN, "ropebert_jina"), device="cuda", model_kwargs={"tokenizer": HashTokenizer("xlmr", 600)})


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_bad_arguments_refused_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.ropebert import _RbLayerW, _RbW

    lib, st = _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream
    fwd, wsb = (getattr(lib, n + sfx) for n in ("tt_ropebert_forward", "tt_ropebert_workspace_bytes"))
    layers = (_RbLayerW * 1)()

    def weights(**kw):
        a = dict(hidden=768, layers=1, heads=12, ffn=3072, vocab=1000, type_vocab=2, mlp_kind=1, ln_eps=1e-12, rope_theta=1000.0,
                 word_emb=1, type_emb=1, emb_ln_g=1, emb_ln_b=1)
        a.update(kw)
        return _RbW(layer=ctypes.cast(layers, ctypes.POINTER(_RbLayerW)), **a)

    def err():
        return lib.tt_last_error().decode()

    assert wsb(ctypes.byref(weights()), 256) > 0 and wsb(ctypes.byref(weights(mlp_kind=0)), 256) > 0
    for kw, text in ((dict(hidden=200, heads=3), "hidden=200"), (dict(hidden=1152, heads=18), "hidden=1152"),
                     (dict(hidden=768, heads=24), "head_dim"), (dict(hidden=256, heads=8), "head_dim"), (dict(ffn=100), "ffn=100"),
                     (dict(ffn=192, mlp_kind=0), "ffn=192"), (dict(mlp_kind=2), "mlp_kind=2")):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        rc = fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc == -2 and text in err(), (kw, rc, err())
    assert wsb(ctypes.byref(weights(ffn=192)), 256) > 0          # SwiGLU: the up-projection is 2 x 192 columns wide
    for kw in (dict(word_emb=None), dict(type_emb=None), dict(rope_theta=0.0), dict(ln_eps=0.0)):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        assert fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st) == -1, kw
    w = weights(layers=0)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    need = wsb(ctypes.byref(w), 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = fwd(ctypes.byref(w), p, p, p, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "type_ids" in err()
    rc = fwd(ctypes.byref(w), p, p, None, None, p, 4, 256, 16, p, base, need, st)          # NULL seq_start
    assert rc == -1 and "null pointer" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 0, 256, 16, p, base, need, st)
    assert rc == -1 and "n_seq" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 200, 16, p, base, need, st)
    assert rc == -1 and "n_rows" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need - 1, st)         # a workspace one byte short
    assert rc != 0 and "workspace" in err()
    # a layer with a missing matrix, and a SwiGLU layer that brings an MLP bias
    w = weights()
    assert wsb(ctypes.byref(w), 256) == need
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "null weight" in err()
    for f in ("qkv_w", "o_w", "ln1_g", "ln1_b", "up_w", "down_w", "ln2_g", "ln2_b", "up_b"):
        setattr(layers[0], f, 1)
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "SwiGLU" in err()
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0                      # nothing was launched: the output buffer is untouched
