"""Writes the T5 encoder fixtures under tests/golden/ (run on a machine with transformers; CPU, nothing downloaded):

  t5_mean_dense_l2/            a seeded ``T5EncoderModel`` checkpoint directory (d_model 256, 4 heads of 64, d_ff 512, 2 layers,
                               feed_forward_proj "relu", vocab 600, layer_norm_epsilon 1e-6): config.json, sharded
                               model.safetensors (every file under 1 MiB), modules.json, 1_Pooling/config.json (mean),
                               2_Dense/ (256 -> 128, no bias, Identity) and sentence_bert_config.json (max_seq_length 512).
  t5_gated_mean_dense_l2/      its one-layer "gated-gelu" sibling (T5 v1.1 / flan: wi_0, wi_1, gelu_new).
  Weight scales: unit-scale embeddings (T5's own initialisation: nothing normalises them), a bias table drawn with sigma 3 (the
  published tables span several units; the default initialisation is a bias no test could see), the q projection sharpened 3 x
  so that the attention is not flat, norm weights 1 +- 0.1.
  <name>_expected.npz          token ids (flat ``ids`` + ``lens``: 1, 9, 17, 92, 130, 300 and 510 tokens, each closed by </s>) and,
                               from the model in fp64, one sequence per call (no padding enters):
                               ``emb``       Pooling(mean) -> Dense -> Normalize of the last hidden states,
                               ``e_bf16``    transformers' own error when the model runs in bfloat16 on the CPU: the largest
                                             deviation of its last hidden states from the fp64 ones over all sequences,
                               ``defects``, ``defect_idx`` and ``<defect>_<k>``: the last hidden states (fp64 arithmetic) of
                               sequence ``defect_idx[k]`` under the defects an implementation could have --
                                 ``nobias``      the relative-position bias dropped,
                                 ``mirrored``    the bias of bucket(query - key) instead of bucket(key - query),
                                 ``nexthead``    head h reading head h + 1's column of the table,
                                 ``div8``        the scores divided by sqrt(d_kv) = 8 (T5 does not scale them),
                                 ``block0only``  the bias added in block 0 only (two-layer fixture only),
                                 ``layernorm``   a mean-subtracting LayerNorm in place of T5LayerNorm,
                                 ``nofinalnorm`` the final norm skipped,
                               and ``nodense_emb``: the embeddings with the Dense module skipped (the normalised mean, cut to the
                               Dense module's width).
  <name>_hidden.npz, <name>_hidden_510.npz
                               ``hidden_<i>``: the fp64 last hidden state of sequence i (stored as fp32; the 510-token sequence in
                               the second file, to keep every file under 1 MiB).

The fp64 states come from this file's own restatement of modeling_t5.py (``forward64``), which is first held against
transformers' ``T5EncoderModel`` in fp64 (they agree to 1e-5: transformers' T5LayerNorm keeps its statistics in fp32 even
there) -- the defects are switches of the restatement.

The GPU test bounds |hidden_hip - hidden_fp64| by 2 e_bf16 (the factor the MPNet, ModernBERT and Gemma tests give a second 16-bit
implementation) and wants every defect reference outside that bound.  An implementation within 2 e of the fp64 states is more
than 2 e away from a defect iff the defect is more than 4 e away from them: asserted below for every defect.

    python tests/golden/make_t5_golden.py
"""
import copy
import json
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB, PAD, EOS, FIRST_WORD = 600, 0, 1, 3
LENGTHS = [1, 9, 17, 92, 130, 300, 510]
DEFECT_LENGTHS = [9, 17, 92]
SEED = 43
BIAS_STD = 3.0
Q_SHARPEN = 3.0
FACTOR = 2.0          # the GPU test's head-room over e_bf16
D_MODEL, HEADS, D_FF, DENSE_OUT, EPS = 256, 4, 512, 128, 1e-6
REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
FIXTURES = (("t5_mean_dense_l2", 2, "relu"), ("t5_gated_mean_dense_l2", 1, "gated-gelu"))
DEFECTS = ("nobias", "mirrored", "nexthead", "div8", "block0only", "layernorm", "nofinalnorm")


def sequences(rng):
    """words </s>; a single token is </s> alone.  No <pad> (id 0): packed batches hold none."""
    out = []
    for n in LENGTHS:
        s = rng.integers(FIRST_WORD, VOCAB, n).astype(np.int32)
        s[-1] = EOS
        out.append(s)
    return out


def forward64(sd, ids, layers, gated, defect=None):
    """modeling_t5.py's encoder stack in fp64 on one sequence -> last hidden state [n][d_model]; ``defect``: see the module text."""
    from transformers.models.t5.modeling_t5 import T5Attention

    n = len(ids)
    h = sd["shared.weight"][torch.from_numpy(ids.astype(np.int64))]
    i = torch.arange(n, dtype=torch.long)
    rel = i[None, :] - i[:, None]                      # memory (key) - context (query)
    bucket = T5Attention._relative_position_bucket(-rel if defect == "mirrored" else rel, bidirectional=True, num_buckets=32,
                                                   max_distance=128)
    bias = sd[REL][bucket].permute(2, 0, 1)            # [heads][query][key]
    if defect == "nexthead":
        bias = bias.roll(-1, dims=0)
    if defect == "nobias":
        bias = torch.zeros_like(bias)

    def norm(x, w):
        if defect == "layernorm":
            x = x - x.mean(-1, keepdim=True)
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w

    def heads_of(x):
        return x.view(n, HEADS, 64).transpose(0, 1)

    for l in range(layers):
        a, m = f"encoder.block.{l}.layer.0.", f"encoder.block.{l}.layer.1."
        x = norm(h, sd[a + "layer_norm.weight"])
        q, k, v = (heads_of(x @ sd[a + f"SelfAttention.{t}.weight"].T) for t in "qkv")
        s = q @ k.transpose(1, 2)
        if defect == "div8":
            s = s / 8.0
        if not (defect == "block0only" and l > 0):
            s = s + bias
        ctx = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(n, D_MODEL)
        h = h + ctx @ sd[a + "SelfAttention.o.weight"].T
        x = norm(h, sd[m + "layer_norm.weight"])
        if gated:
            g = x @ sd[m + "DenseReluDense.wi_0.weight"].T
            g = 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g.pow(3))))
            f = g * (x @ sd[m + "DenseReluDense.wi_1.weight"].T)
        else:
            f = torch.relu(x @ sd[m + "DenseReluDense.wi.weight"].T)
        h = h + f @ sd[m + "DenseReluDense.wo.weight"].T
    return h if defect == "nofinalnorm" else norm(h, sd["encoder.final_layer_norm.weight"])


def hidden_of(model, ids):
    with torch.no_grad():
        return model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0]


def write_fixture(name, layers, ffp, seqs):
    from safetensors.torch import load_file, save_file
    from transformers import T5Config, T5EncoderModel

    cfg = T5Config(vocab_size=VOCAB, d_model=D_MODEL, d_kv=64, d_ff=D_FF, num_layers=layers, num_heads=HEADS,
                   relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0,
                   layer_norm_epsilon=EPS, feed_forward_proj=ffp, is_encoder_decoder=False, use_cache=False,
                   pad_token_id=PAD, eos_token_id=EOS)
    model = T5EncoderModel(cfg).eval().to(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("layer_norm.weight"):
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif n.endswith("SelfAttention.q.weight"):
                p.mul_(Q_SHARPEN)
            elif n.endswith("relative_attention_bias.weight"):
                p.copy_(BIAS_STD * torch.randn_like(p))
    dense = torch.randn(DENSE_OUT, D_MODEL) * D_MODEL ** -0.5

    d = os.path.join(HERE, name)
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    os.makedirs(os.path.join(d, "2_Dense"), exist_ok=True)
    model.save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
    for stray in ("generation_config.json",):
        if os.path.exists(os.path.join(d, stray)):
            os.remove(os.path.join(d, stray))
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Dense", "type": "sentence_transformers.models.Dense"},
                   {"idx": 3, "name": "3", "path": "3_Normalize", "type": "sentence_transformers.models.Normalize"}], f, indent=2)
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": D_MODEL, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
                   "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
                   "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": False, "include_prompt": True}, f, indent=2)
    with open(os.path.join(d, "2_Dense", "config.json"), "w") as f:
        json.dump({"in_features": D_MODEL, "out_features": DENSE_OUT, "bias": False,
                   "activation_function": "torch.nn.modules.linear.Identity"}, f, indent=2)
    save_file({"linear.weight": dense.contiguous()}, os.path.join(d, "2_Dense", "model.safetensors"))
    with open(os.path.join(d, "sentence_bert_config.json"), "w") as f:
        json.dump({"max_seq_length": 512, "do_lower_case": False}, f, indent=2)
    with open(os.path.join(d, "config.json")) as f:
        saved = json.load(f)
    assert saved["model_type"] == "t5" and saved["architectures"] == ["T5EncoderModel"] and saved["feed_forward_proj"] == ffp
    idx = os.path.join(d, "model.safetensors.index.json")
    if os.path.exists(idx):
        with open(idx) as f:
            shards = sorted(set(json.load(f)["weight_map"].values()))
    else:
        shards = ["model.safetensors"]
    stored = {}
    for s in shards:
        stored.update(load_file(os.path.join(d, s)))
    assert REL in stored and ("shared.weight" in stored or "encoder.embed_tokens.weight" in stored), sorted(stored)[:8]
    assert not any(k.startswith(("decoder.", "lm_head")) for k in stored)

    m64 = copy.deepcopy(model).double()
    sd = {k: v.double() for k, v in model.state_dict().items()}
    gated = ffp == "gated-gelu"
    hidden = [forward64(sd, s, layers, gated) for s in seqs]
    hf = [hidden_of(m64, s) for s in seqs]
    agree = max(float((a - b).abs().max()) for a, b in zip(hidden, hf))
    # (not 1e-12: T5LayerNorm takes its mean of squares in fp32 whatever the model's type -- 6e-8 relative in every norm)
    assert agree < 1e-5, f"the restatement and transformers differ by {agree}"
    d64 = dense.double()

    def tail(h, with_dense=True):
        p = h.mean(0)
        v = d64 @ p if with_dense else p
        return torch.nn.functional.normalize(v, dim=0)

    emb = np.stack([tail(h).numpy() for h in hidden])
    nodense = np.stack([tail(h, False).numpy()[:DENSE_OUT] for h in hidden])
    nodense /= np.linalg.norm(nodense, axis=1, keepdims=True)
    cos_nodense = float((emb * nodense).sum(1).max())
    assert cos_nodense < 0.9, f"the Dense-skipped embeddings are at cos {cos_nodense} of the right ones"
    m16 = copy.deepcopy(model).to(torch.bfloat16)          # cast afresh from the fp32 weights
    e_bf16 = max(float((hidden_of(m16, s).double() - h).abs().max()) for s, h in zip(seqs, hidden))
    assert 1e-4 < e_bf16 < 0.5, e_bf16

    names = [x for x in DEFECTS if not (x == "block0only" and layers < 2)]
    defect_idx = [LENGTHS.index(n) for n in DEFECT_LENGTHS]
    defects, gaps = {}, {}
    for x in names:
        for k, i in enumerate(defect_idx):
            defects[f"{x}_{k}"] = forward64(sd, seqs[i], layers, gated, defect=x)
        gaps[x] = max(float((defects[f"{x}_{k}"] - hidden[i]).abs().max()) for k, i in enumerate(defect_idx))
        assert gaps[x] > 2 * FACTOR * e_bf16, (f"{name}: defect '{x}' is only {gaps[x]:.4f} from the fp64 states: inside 2 x the "
                                               f"test's bound {FACTOR} x e_bf16 = {FACTOR * e_bf16:.4f}")

    np.savez_compressed(os.path.join(HERE, f"{name}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(LENGTHS, dtype=np.int32),
                        emb=emb.astype(np.float64), nodense_emb=nodense.astype(np.float64), e_bf16=np.float64(e_bf16),
                        defects=np.asarray(names), defect_idx=np.asarray(defect_idx, dtype=np.int32),
                        **{k: v.numpy().astype(np.float32) for k, v in defects.items()})
    small = {f"hidden_{i}": h.numpy().astype(np.float32) for i, h in enumerate(hidden) if LENGTHS[i] != 510}
    np.savez_compressed(os.path.join(HERE, f"{name}_hidden.npz"), **small)
    i510 = LENGTHS.index(510)
    np.savez_compressed(os.path.join(HERE, f"{name}_hidden_510.npz"), **{f"hidden_{i510}": hidden[i510].numpy().astype(np.float32)})
    for root, _, files in os.walk(d):
        for fn in files:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for sfx in ("expected", "hidden", "hidden_510"):
        assert os.path.getsize(os.path.join(HERE, f"{name}_{sfx}.npz")) < 1 << 20, sfx
    print(name, "written: e_bf16", round(e_bf16, 5), "defect gaps", {k: round(v, 3) for k, v in gaps.items()},
          "Dense-skipped cos", round(cos_nodense, 3), "hidden abs max", round(max(float(h.abs().max()) for h in hidden), 3))


def main():
    torch.manual_seed(SEED)
    seqs = sequences(np.random.default_rng(SEED))
    assert [len(s) for s in seqs] == LENGTHS
    for name, layers, ffp in FIXTURES:
        write_fixture(name, layers, ffp, seqs)


if __name__ == "__main__":
    main()
