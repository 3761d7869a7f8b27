"""Writes the NomicBERT / Jina-embeddings-v3 fixtures under tests/golden/ (run on a machine with transformers; CPU, nothing
downloaded):

  ropebert_nomic/              a seeded ``NomicBertModel`` checkpoint directory (hidden 256, 4 heads of 64, intermediate_size 512, 2
                               layers, vocab 600, type_vocab_size 2, 2048 positions, rope_theta 1000, SwiGLU, no biases): config.json,
                               sharded model.safetensors, modules.json and 1_Pooling/config.json (mean).
  ropebert_jina/               a seeded ``JinaEmbeddingsV3Model`` of the same sizes (type_vocab_size 1, rope_theta 20000, pad_token_id
                               1, GELU MLP, biases everywhere; the ``pooler.*`` tensors are present, as the class writes them).
  ropebert_nomic_orig/         the NomicBERT weights a second time in the ORIGINAL tensor layout -- ``encoder.layers.N.attn.Wqkv``,
                               ``attn.out_proj``, ``mlp.fc11`` (up) / ``fc12`` (gate) / ``fc2`` (down), ``norm1`` / ``norm2``,
                               ``emb_ln`` -- built by inverting the renamings transformers/conversion_mapping.py lists for
                               "nomic_bert" and asserted equal to what ``save_pretrained`` writes (transformers saves these two
                               types in the original layout); its config.json is the transformers-format one.
                               The weights are rounded to fp16 before anything is computed and stored as fp16 (every file under
                               1 MiB), with trained-model-like scales: q / k sharpened (at +-0.02 the attention is uniform and RoPE
                               invisible), biases and LayerNorm biases of the order of the activations, token-type row 0 non-zero.
  ropebert_<name>_expected.npz token ids (flat ``ids`` + ``lens``: 1, 9, 17, 92, 130, 300 and 700 tokens) and, from the transformers
                               model in fp64, one sequence per call (no padding enters):
                               ``emb``                 the mean-pooled, L2-normalised last hidden states,
                               ``e_bf16`` / ``e_fp16`` the same model's own error when it runs in that type on the CPU: the largest
                                                       deviation of its last hidden states from the fp64 ones over all sequences,
                               ``defect_idx``, ``defects``, ``defects_fp16_only``: see below.
  ropebert_<name>_defect_<defect>.npz
                               ``<defect>_<k>``: the last hidden states (fp64 arithmetic, the layer restated below and checked
                               against the model; stored as fp32, one file per defect to keep every file under 1 MiB) of sequence
                               ``defect_idx[k]`` (9, 92 and 300 tokens) under the defects an implementation could have --
                                 ``norope``       q and k not rotated,
                                 ``interleaved``  the pairs (2i, 2i + 1) rotated instead of (i, i + 32) (rotate-half),
                                 ``theta``        RoPE base 10000 in place of the config's,
                                 ``swapglu``      SiLU applied to up_proj instead of gate_proj (nomic only),
                                 ``notype``       token-type row 0 not added,
                                 ``prenorm``      the LayerNorm in front of each sublayer instead of behind the residual sum,
                                 ``nobias``       the q / k / v biases dropped (jina only).
                               A defect less than 4 e_bf16 from the fp64 states is listed in ``defects_fp16_only``.
  ropebert_<name>_hidden.npz, ropebert_<name>_hidden_700.npz
                               ``hidden_<i>``: the fp64 last hidden state of sequence i (stored as fp32; the 700-token sequence in
                               the second file, to keep every file under 1 MiB).

The GPU test bounds |hidden_hip - hidden_fp64| by 2 e_<type> (the factor the ModernBERT, Gemma, MPNet and DeBERTa tests give a second
16-bit implementation) and wants every defect reference outside that bound.  An implementation within 2 e of the fp64 states is more
than 2 e away from a defect iff the defect is more than 4 e away from them: asserted below for every defect used for a type.

    python tests/golden/make_ropebert_golden.py
"""
import copy
import json
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB, FIRST, LAST, FIRST_WORD = 600, 2, 3, 4       # ids 0 and 1 (the two pad ids) never occur: packed batches hold no padding
LENGTHS = [1, 9, 17, 92, 130, 300, 700]
DEFECT_LENGTHS = [9, 92, 300]
SEED = 53
QK_SHARPEN = 5.0
VO_GAIN = 3.0         # v_proj and o_proj: an attention sublayer whose output is of the order of the residual stream, as trained ones are
TYPE_STD = 0.05       # token-type rows: of the order of the word embeddings
BIAS_STD = 0.3        # projection biases (jina): of the order of the projections' outputs
LN_BIAS_STD = 0.1
MLP_GAIN = (3.0, 2.0)  # gate / up / fc1, and down / fc2: an MLP whose gate leaves SiLU's linear range
FACTOR = 2.0          # the GPU test's head-room over e_<type>
HIDDEN, HEADS, FFN, LAYERS, MAX_POS = 256, 4, 512, 2, 2048
FP16_ONLY = {"nomic": [], "jina": []}


def sequences(rng):
    out = []
    for n in LENGTHS:
        s = rng.integers(FIRST_WORD, VOCAB, n).astype(np.int32)
        s[0] = FIRST
        if n > 1:
            s[-1] = LAST
        out.append(s)
    return out


def hidden_of(model, ids):
    with torch.no_grad():
        return model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0]


def cast(model, dt):
    """A copy of ``model`` with its parameters in ``dt`` and the rotary module's inverse frequencies left in fp32, as
    ``from_pretrained(dtype=dt)`` leaves them (``Module.to`` would round that buffer to ``dt`` too: at position 699 a bf16
    frequency is an angle error of more than a radian, which no implementation of the model has)."""
    m = copy.deepcopy(model).to(dt)
    for name in ("inv_freq", "original_inv_freq"):
        setattr(m.rotary_emb, name, getattr(model.rotary_emb, name).detach().clone().to(torch.float32))
    return m


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def forward64(sd, kind, theta, eps, ids, defect=None):
    """The model restated in fp64 on the state dict ``sd`` (transformers names), with one defect switched on.  cos / sin are
    computed as the rotary module computes them (fp32 inverse frequencies and angles), then used in fp64."""
    n = len(ids)
    lin = lambda x, name: x @ sd[name + ".weight"].T + (sd[name + ".bias"] if name + ".bias" in sd else 0.0)  # noqa: E731
    x = sd["embeddings.word_embeddings.weight"][torch.from_numpy(ids.astype(np.int64))]
    if defect != "notype":
        x = x + sd["embeddings.token_type_embeddings.weight"][0]
    x = layer_norm(x, sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], eps)
    base = 10000.0 if defect == "theta" else theta
    inv = 1.0 / (base ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64))
    ang = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]           # [n][32] fp32
    cos, sin = ang.cos().double(), ang.sin().double()

    def rope(t):                                   # t [n][heads][64]
        if defect == "norope":
            return t
        c, s = cos[:, None, :], sin[:, None, :]
        if defect == "interleaved":
            a, b = t[..., 0::2], t[..., 1::2]
            out = torch.empty_like(t)
            out[..., 0::2], out[..., 1::2] = a * c - b * s, b * c + a * s
            return out
        a, b = t[..., :32], t[..., 32:]
        return torch.cat([a * c - b * s, b * c + a * s], -1)

    def attention(h, p):
        q, k, v = (lin(h, p + f"self_attn.{m}_proj") for m in "qkv")
        if defect == "nobias":
            q, k, v = (h @ sd[p + f"self_attn.{m}_proj.weight"].T for m in "qkv")
        q, k, v = (t.view(n, HEADS, 64) for t in (q, k, v))
        q, k = rope(q), rope(k)
        s = torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(64)
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, HIDDEN)
        return lin(a, p + "self_attn.o_proj")

    def mlp(h, p):
        if kind == "nomic":
            g, u = lin(h, p + "mlp.gate_proj"), lin(h, p + "mlp.up_proj")
            if defect == "swapglu":
                g, u = u, g
            return lin(torch.nn.functional.silu(g) * u, p + "mlp.down_proj")
        return lin(torch.nn.functional.gelu(lin(h, p + "mlp.fc1")), p + "mlp.fc2")

    for i in range(LAYERS):
        p = f"layers.{i}."
        ln1 = lambda t: layer_norm(t, sd[p + "post_attention_layernorm.weight"], sd[p + "post_attention_layernorm.bias"], eps)  # noqa: E731
        ln2 = lambda t: layer_norm(t, sd[p + "post_mlp_layernorm.weight"], sd[p + "post_mlp_layernorm.bias"], eps)  # noqa: E731
        if defect == "prenorm":
            x = x + attention(ln1(x), p)
            x = x + mlp(ln2(x), p)
        else:
            x = ln1(x + attention(x, p))
            x = ln2(x + mlp(x, p))
    return x


def to_original_layout(sd):
    """Transformers names -> the original NomicBERT layout: the renamings of conversion_mapping.py["nomic_bert"] inverted, q / k / v
    concatenated along dim 0 into Wqkv."""
    out = {}
    for k, v in sd.items():
        if ".self_attn.k_proj." in k or ".self_attn.v_proj." in k:
            continue
        if ".self_attn.q_proj." in k:
            out[k.replace("layers.", "encoder.layers.").replace("self_attn.q_proj", "attn.Wqkv")] = torch.cat(
                [sd[k.replace("q_proj", m + "_proj")] for m in "qkv"], 0)
            continue
        for new, old in (("embeddings.LayerNorm", "emb_ln"), ("self_attn.o_proj", "attn.out_proj"), ("up_proj", "fc11"),
                         ("gate_proj", "fc12"), ("down_proj", "fc2"), ("post_attention_layernorm", "norm1"),
                         ("post_mlp_layernorm", "norm2")):
            k = k.replace(new, old)
        if k.startswith("layers."):
            k = "encoder." + k
        out[k] = v
    return out


def write_sharded(d, sd, limit=900_000):
    from safetensors.torch import save_file

    shards, cur, size = [], {}, 0
    for k, v in sd.items():
        nb = v.numel() * v.element_size()
        if cur and size + nb > limit:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = v.contiguous()
        size += nb
    shards.append(cur)
    weight_map = {}
    for i, sh in enumerate(shards):
        fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
        save_file(sh, os.path.join(d, fn), metadata={"format": "pt"})
        weight_map.update({k: fn for k in sh})
    with open(os.path.join(d, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {"total_size": sum(v.numel() * v.element_size() for v in sd.values())}, "weight_map": weight_map}, f,
                  indent=2)


def sentence_transformers_files(d):
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}], f, indent=2)
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": HIDDEN, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
                   "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
                   "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": False, "include_prompt": True}, f, indent=2)


def build(kind):
    from transformers import JinaEmbeddingsV3Config, JinaEmbeddingsV3Model, NomicBertConfig, NomicBertModel

    name = f"ropebert_{kind}"
    torch.manual_seed(SEED + (0 if kind == "nomic" else 1))
    common = dict(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=FFN, num_hidden_layers=LAYERS,
                  max_position_embeddings=MAX_POS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    if kind == "nomic":
        cfg = NomicBertConfig(type_vocab_size=2, **common)
        model = NomicBertModel(cfg)
        theta = 1000.0
    else:
        cfg = JinaEmbeddingsV3Config(type_vocab_size=1, pad_token_id=1, **common)
        model = JinaEmbeddingsV3Model(cfg)
        theta = 20000.0
    assert cfg.rope_parameters["rope_theta"] == theta and cfg.rope_parameters["rope_type"] == "default"
    eps = cfg.layer_norm_eps
    model = model.eval().to(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():       # trained-model-like scales: nothing exactly 1 or exactly 0
            if "LayerNorm.weight" in n or "layernorm.weight" in n:
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif "LayerNorm.bias" in n or "layernorm.bias" in n:
                p.copy_(LN_BIAS_STD * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.copy_(BIAS_STD * torch.randn_like(p))
        emb = model.embeddings
        emb.word_embeddings.weight[cfg.pad_token_id].copy_(0.02 * torch.randn(HIDDEN))      # Embedding(padding_idx=) zeroed this row
        emb.token_type_embeddings.weight.copy_(TYPE_STD * torch.randn_like(emb.token_type_embeddings.weight))
        for layer in model.layers:
            for lin in (layer.self_attn.q_proj, layer.self_attn.k_proj):
                lin.weight.mul_(QK_SHARPEN)
            for lin in (layer.self_attn.v_proj, layer.self_attn.o_proj):
                lin.weight.mul_(VO_GAIN)
            mlp = layer.mlp
            for lin in ((mlp.gate_proj, mlp.up_proj) if kind == "nomic" else (mlp.fc1,)):
                lin.weight.mul_(MLP_GAIN[0])
            (mlp.down_proj if kind == "nomic" else mlp.fc2).weight.mul_(MLP_GAIN[1])
        model = cast(model, torch.float16).float()  # the stored weights ARE the model's: fp16 values
    rng = np.random.default_rng(SEED)
    seqs = sequences(rng)
    assert [len(s) for s in seqs] == LENGTHS and max(LENGTHS) <= MAX_POS

    d = os.path.join(HERE, name)
    half = copy.deepcopy(model).half()
    stored = {k: v.clone() for k, v in half.state_dict().items()}          # the transformers names
    assert "layers.0.self_attn.q_proj.weight" in stored and ("layers.0.self_attn.q_proj.bias" in stored) == (kind == "jina")
    assert ("layers.0.mlp.gate_proj.weight" in stored) == (kind == "nomic") and ("layers.0.mlp.fc1.bias" in stored) == (kind == "jina")
    assert ("pooler.dense.weight" in stored) == (kind == "jina") and not any("inv_freq" in k for k in stored)
    assert all(torch.equal(v.float(), model.state_dict()[k]) for k, v in stored.items())
    # save_pretrained writes the ORIGINAL layout (it applies conversion_mapping.py in reverse): that is the second nomic directory,
    # and what ``to_original_layout`` must reproduce; the transformers-layout directories are written here, tensor by tensor
    import tempfile

    from safetensors.torch import load_file

    with tempfile.TemporaryDirectory() as tmp:
        half.save_pretrained(tmp, max_shard_size="900KB", safe_serialization=True)
        with open(os.path.join(tmp, "config.json")) as f:
            saved = json.load(f)
        with open(os.path.join(tmp, "model.safetensors.index.json")) as f:
            shards = sorted(set(json.load(f)["weight_map"].values()))
        as_saved = {}
        for sh in shards:
            as_saved.update(load_file(os.path.join(tmp, sh)))
    assert saved["model_type"] == ("nomic_bert" if kind == "nomic" else "jina_embeddings_v3")
    assert saved["rope_parameters"]["rope_theta"] == theta and saved["hidden_size"] == HIDDEN
    dirs = [(d, stored)]
    if kind == "nomic":
        orig = to_original_layout(stored)
        assert "encoder.layers.1.attn.Wqkv.weight" in orig and "encoder.layers.0.mlp.fc11.weight" in orig and "emb_ln.bias" in orig
        assert not any("self_attn" in k or "layernorm" in k or "LayerNorm" in k for k in orig) and len(orig) == len(stored) - 2 * LAYERS
        assert sorted(orig) == sorted(as_saved) and all(torch.equal(orig[k], as_saved[k]) for k in orig)
        dirs.append((d + "_orig", orig))
    else:
        assert "encoder.layers.0.mixer.Wqkv.weight" in as_saved and "encoder.layers.0.mlp.fc1.weight" in as_saved
    for dd, tensors in dirs:
        os.makedirs(dd, exist_ok=True)
        for fn in os.listdir(dd):                  # (a re-run with another shard count leaves no stale shard behind)
            if fn.endswith(".safetensors"):
                os.remove(os.path.join(dd, fn))
        write_sharded(dd, tensors)
        sentence_transformers_files(dd)
        with open(os.path.join(dd, "config.json"), "w") as f:
            json.dump(saved, f, indent=2)

    m64 = cast(model, torch.float64)
    hidden = [hidden_of(m64, s) for s in seqs]
    emb = np.stack([torch.nn.functional.normalize(h.mean(0), dim=0).numpy() for h in hidden])
    e = {}
    for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m16 = cast(model, dt)                      # cast afresh from the stored weights
        e[key] = max(float((hidden_of(m16, s).double() - h).abs().max()) for s, h in zip(seqs, hidden))
    assert all(1e-4 < v < 0.5 for v in e.values()), e

    sd64 = {k: v.double() for k, v in model.state_dict().items()}
    # the restated layer is the model's
    restated = max(float((forward64(sd64, kind, theta, eps, s) - h).abs().max()) for s, h in zip(seqs, hidden))
    assert restated < 1e-9, restated
    names = ["norope", "interleaved", "theta", "notype", "prenorm"] + (["swapglu"] if kind == "nomic" else ["nobias"])
    defect_idx = [LENGTHS.index(n) for n in DEFECT_LENGTHS]
    defects, gaps = {}, {}
    for dn in names:
        for k, i in enumerate(defect_idx):
            defects[f"{dn}_{k}"] = forward64(sd64, kind, theta, eps, seqs[i], defect=dn)
        gaps[dn] = max(float((defects[f"{dn}_{k}"] - hidden[i]).abs().max()) for k, i in enumerate(defect_idx))
        for key, v in e.items():
            if key == "bf16" and dn in FP16_ONLY[kind]:
                continue
            assert gaps[dn] > 2 * FACTOR * v, (f"{kind}: defect '{dn}' is only {gaps[dn]:.4f} from the fp64 states: inside 2 x the "
                                               f"test's bound {FACTOR} x e_{key} = {FACTOR * v:.4f}; rescale the weights or list it in "
                                               "FP16_ONLY")
    np.savez_compressed(os.path.join(HERE, f"{name}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(LENGTHS, dtype=np.int32),
                        emb=emb.astype(np.float64), e_bf16=np.float64(e["bf16"]), e_fp16=np.float64(e["fp16"]),
                        defect_idx=np.asarray(defect_idx, dtype=np.int32), defects=np.asarray(names),
                        defects_fp16_only=np.asarray(FP16_ONLY[kind], dtype="<U16"))
    for dn in names:
        np.savez_compressed(os.path.join(HERE, f"{name}_defect_{dn}.npz"),
                            **{f"{dn}_{k}": defects[f"{dn}_{k}"].numpy().astype(np.float32) for k in range(len(defect_idx))})
        assert os.path.getsize(os.path.join(HERE, f"{name}_defect_{dn}.npz")) < 1 << 20, dn
    i700 = LENGTHS.index(700)
    np.savez_compressed(os.path.join(HERE, f"{name}_hidden.npz"),
                        **{f"hidden_{i}": h.numpy().astype(np.float32) for i, h in enumerate(hidden) if i != i700})
    np.savez_compressed(os.path.join(HERE, f"{name}_hidden_700.npz"), **{f"hidden_{i700}": hidden[i700].numpy().astype(np.float32)})
    for dd in [d] + ([d + "_orig"] if kind == "nomic" else []):
        for root, _, files in os.walk(dd):
            for fn in files:
                assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for sfx in ("expected", "hidden", "hidden_700"):
        assert os.path.getsize(os.path.join(HERE, f"{name}_{sfx}.npz")) < 1 << 20, sfx
    print(name, "written: e", e, "defect gaps", gaps, "restated", restated, "hidden abs max", max(float(h.abs().max()) for h in hidden))


def main():
    build("nomic")
    build("jina")


if __name__ == "__main__":
    main()
