"""Writes the MPNet fixture under tests/golden/ (run on a machine with transformers; CPU, nothing downloaded):

  mpnet_mean_l2/               a seeded ``MPNetModel`` checkpoint directory (hidden 256, 4 heads of 64, intermediate_size 512, 2
                               layers, vocab 600, 514 positions, layer_norm_eps 1e-5): config.json, sharded model.safetensors (every
                               file under 1 MiB; the ``pooler.*`` tensors are present, as in the published checkpoints),
                               modules.json and 1_Pooling/config.json (mean).  ``relative_attention_bias.weight`` is drawn several
                               units wide, as the published checkpoints' tables are (the default initialisation, +-0.02, is a bias no
                               test could see), and the q / k projections are scaled up so that the attention is not flat.
  mpnet_mean_l2_expected.npz   token ids (flat ``ids`` + ``lens``: 1, 9, 17, 92, 130, 300 and 510 tokens; positions run to 514 - 2 = 512) and,
                               from the model in fp64, one sequence per call (no padding enters):
                               ``emb``                 the mean-pooled, L2-normalised last hidden states,
                               ``e_bf16`` / ``e_fp16`` the same model's own error when it runs in that type on the CPU: the largest
                                                       deviation of its last hidden states from the fp64 ones over all sequences,
                               ``defect_idx`` and ``<defect>_<k>``: the last hidden states (fp64 arithmetic) of sequence
                               ``defect_idx[k]`` under five defects an implementation could have --
                                 ``nobias``    the relative-position bias dropped,
                                 ``mirrored``  the bias of bucket(query - key) instead of bucket(key - query),
                                 ``shifted``   the bias table shifted one row (query i gets the bias row of query i + 1),
                                 ``nexthead``  head h reading head h + 1's column of the table,
                                 ``pos0``      positions starting at 0 instead of padding_idx + 1 = 2.
  mpnet_mean_l2_hidden.npz, mpnet_mean_l2_hidden_510.npz
                               ``hidden_<i>``: the fp64 last hidden state of sequence i (stored as fp32; the 510-token sequence in
                               the second file, to keep every file under 1 MiB).

The GPU test bounds |hidden_hip - hidden_fp64| by 2 e_<type> (the factor the ModernBERT and Gemma tests give a second 16-bit
implementation) and wants every defect reference outside that bound.  An implementation within 2 e of the fp64 states is more than
2 e away from a defect iff the defect is more than 4 e away from them: asserted below for every defect, in both types.

    python tests/golden/make_mpnet_golden.py
"""
import copy
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "mpnet_mean_l2"
VOCAB, BOS, PAD, EOS, FIRST_WORD = 600, 0, 1, 2, 4
LENGTHS = [1, 9, 17, 92, 130, 300, 510]
DEFECT_LENGTHS = [9, 17, 92]
SEED = 41
BIAS_STD = 3.0        # the published tables span several units
QK_SHARPEN = 5.0
FACTOR = 2.0          # the GPU test's head-room over e_<type>


def sequences(rng):
    """<s> words </s>; a single token is <s> alone.  No <pad> (id 1): packed batches hold none."""
    out = []
    for n in LENGTHS:
        s = rng.integers(FIRST_WORD, VOCAB, n).astype(np.int32)
        s[0] = BOS
        if n > 1:
            s[-1] = EOS
        out.append(s)
    return out


def hidden_of(model, ids, position_ids=None):
    with torch.no_grad():
        t = torch.from_numpy(ids.astype(np.int64))[None]
        return model(input_ids=t, position_ids=position_ids).last_hidden_state[0]


def with_bias(model, patch):
    """A copy of ``model`` whose position bias [1][heads][q][k] is ``patch(encoder, x)``."""
    m = copy.deepcopy(model)
    enc = m.encoder
    enc.compute_position_bias = lambda x, position_ids=None, num_buckets=32: patch(enc, x)
    return m


def bias_from(enc, x, relative_position):
    n = x.size(1)
    values = enc.relative_attention_bias(enc.relative_position_bucket(relative_position(n), num_buckets=32))
    return values.permute([2, 0, 1]).unsqueeze(0).expand((x.size(0), -1, n, n)).contiguous()


def _rel(n, sign=1, shift=0):
    i = torch.arange(n, dtype=torch.long)
    return sign * (i[None, :] - i[:, None]) - shift          # memory (key) - context (query)


def main():
    from transformers import MPNetConfig, MPNetModel

    torch.manual_seed(SEED)
    cfg = MPNetConfig(vocab_size=VOCAB, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2,
                      max_position_embeddings=514, layer_norm_eps=1e-5, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = MPNetModel(cfg).eval().to(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():       # trained-model-like scales: nothing exactly 1 or exactly 0
            if n.endswith("LayerNorm.weight"):
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif n.endswith("LayerNorm.bias"):
                p.copy_(0.05 * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.copy_(0.02 * torch.randn_like(p))
        # Embedding(padding_idx=) zeroed this row; trained checkpoints carry ordinary values there
        model.embeddings.word_embeddings.weight[PAD].copy_(0.02 * torch.randn(cfg.hidden_size))
        model.embeddings.position_embeddings.weight[PAD].copy_(0.02 * torch.randn(cfg.hidden_size))
        model.encoder.relative_attention_bias.weight.copy_(BIAS_STD * torch.randn(32, cfg.num_attention_heads))
        for layer in model.encoder.layer:
            for lin in (layer.attention.attn.q, layer.attention.attn.k):
                lin.weight.mul_(QK_SHARPEN)
                lin.bias.mul_(QK_SHARPEN)
    rng = np.random.default_rng(SEED)
    seqs = sequences(rng)
    assert [len(s) for s in seqs] == LENGTHS and max(LENGTHS) <= cfg.max_position_embeddings - (PAD + 1)

    d = os.path.join(HERE, NAME)
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    model.save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}], f, indent=2)
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": 256, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
                   "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
                   "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": False, "include_prompt": True}, f, indent=2)
    with open(os.path.join(d, "config.json")) as f:
        saved = json.load(f)
    assert saved["model_type"] == "mpnet" and saved["architectures"] == ["MPNetModel"] and saved["relative_attention_num_buckets"] == 32
    from safetensors.torch import load_file

    with open(os.path.join(d, "model.safetensors.index.json")) as f:
        shards = sorted(set(json.load(f)["weight_map"].values()))
    names = set().union(*(load_file(os.path.join(d, s)).keys() for s in shards))
    assert {"pooler.dense.weight", "pooler.dense.bias", "encoder.relative_attention_bias.weight"} <= names
    assert "encoder.layer.0.attention.attn.q.weight" in names and not any(n.startswith("mpnet.") for n in names)

    m64 = copy.deepcopy(model).double()
    hidden = [hidden_of(m64, s) for s in seqs]
    emb = np.stack([torch.nn.functional.normalize(h.mean(0), dim=0).numpy() for h in hidden])
    e = {}
    for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m16 = copy.deepcopy(model).to(dt)          # cast afresh from the fp32 weights
        e[key] = max(float((hidden_of(m16, s).double() - h).abs().max()) for s, h in zip(seqs, hidden))
    assert all(1e-4 < v < 0.5 for v in e.values()), e

    defect_models = {
        "nobias": with_bias(m64, lambda enc, x: torch.zeros(x.size(0), cfg.num_attention_heads, x.size(1), x.size(1), dtype=x.dtype)),
        "mirrored": with_bias(m64, lambda enc, x: bias_from(enc, x, lambda n: _rel(n, sign=-1))),
        "shifted": with_bias(m64, lambda enc, x: bias_from(enc, x, lambda n: _rel(n, shift=1))),
        "nexthead": with_bias(m64, lambda enc, x: bias_from(enc, x, _rel).roll(-1, dims=1)),
    }
    # the patched bias of the unpatched rule is the model's own: the patching itself changes nothing
    same = with_bias(m64, lambda enc, x: bias_from(enc, x, _rel))
    assert all(torch.equal(hidden_of(same, s), h) for s, h in zip(seqs, hidden))
    defect_idx = [LENGTHS.index(n) for n in DEFECT_LENGTHS]
    defects = {}
    for name, m in defect_models.items():
        for k, i in enumerate(defect_idx):
            defects[f"{name}_{k}"] = hidden_of(m, seqs[i])
    for k, i in enumerate(defect_idx):
        defects[f"pos0_{k}"] = hidden_of(m64, seqs[i], position_ids=torch.arange(len(seqs[i]), dtype=torch.long)[None])
    gaps = {}
    for name in list(defect_models) + ["pos0"]:
        gaps[name] = max(float((defects[f"{name}_{k}"] - hidden[i]).abs().max()) for k, i in enumerate(defect_idx))
        for key, v in e.items():
            assert gaps[name] > 2 * FACTOR * v, (f"defect '{name}' is only {gaps[name]:.4f} from the fp64 states: inside "
                                                 f"2 x the test's bound {FACTOR} x e_{key} = {FACTOR * v:.4f}; widen BIAS_STD")

    np.savez_compressed(os.path.join(HERE, f"{NAME}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(LENGTHS, dtype=np.int32),
                        emb=emb.astype(np.float64), e_bf16=np.float64(e["bf16"]), e_fp16=np.float64(e["fp16"]),
                        defect_idx=np.asarray(defect_idx, dtype=np.int32), **{k: v.numpy().astype(np.float32) for k, v in defects.items()})
    small = {f"hidden_{i}": h.numpy().astype(np.float32) for i, h in enumerate(hidden) if LENGTHS[i] != 510}
    np.savez_compressed(os.path.join(HERE, f"{NAME}_hidden.npz"), **small)
    i510 = LENGTHS.index(510)
    np.savez_compressed(os.path.join(HERE, f"{NAME}_hidden_510.npz"), **{f"hidden_{i510}": hidden[i510].numpy().astype(np.float32)})
    for root, _, files in os.walk(d):
        for fn in files:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for sfx in ("expected", "hidden", "hidden_510"):
        assert os.path.getsize(os.path.join(HERE, f"{NAME}_{sfx}.npz")) < 1 << 20, sfx
    print(NAME, "written: e", e, "defect gaps", gaps, "hidden abs max", max(float(h.abs().max()) for h in hidden))


if __name__ == "__main__":
    main()
