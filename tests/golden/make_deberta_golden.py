"""Writes the DeBERTa-v3 cross-encoder fixture under tests/golden/ (run on a machine with transformers; CPU, nothing downloaded):

  deberta_v3_ce/               a seeded ``DebertaV2ForSequenceClassification`` checkpoint directory (hidden 256, 4 heads of 64,
                               intermediate_size 512, 2 layers, vocab 600, 512 positions, position_buckets 256,
                               max_relative_positions -1, share_att_key, pos_att_type ["p2c", "c2p"], norm_rel_ebd "layer_norm",
                               position_biased_input false, type_vocab_size 0, layer_norm_eps 1e-7, one label): config.json and
                               sharded model.safetensors (every file under 1 MiB).  The weights have trained-model-like scales: the
                               default initialisation (+-0.02) leaves both position terms, the LayerNorm of the relative embeddings
                               and the logits below 16-bit noise, where no test could see them.  ``rel_embeddings`` = REL_MEAN +
                               REL_STD randn, ``encoder.LayerNorm.weight`` x REL_LN_GAIN, the query / key projections x QK_SHARPEN,
                               and the classifier scaled until the fp64 logits of the stored sequences spread over LOGIT_SPREAD.
  deberta_v3_ce_expected.npz   token ids (flat ``ids`` + ``lens``: 1, 9, 17, 92, 130, 300 and 510 tokens; [CLS] first, [SEP] last, an
                               inner [SEP] in the pair-shaped ones, no [PAD]) and, from the model in fp64, one sequence per call (no
                               padding enters):
                               ``logits``                    the classifier's output,
                               ``e_bf16`` / ``e_fp16``       the same model's own error when it runs in that type on the CPU: the
                                                             largest deviation of its last hidden states from the fp64 ones,
                               ``logits_bf16`` / ``_fp16``   that run's logits,
                               ``dist_index``                clamp(bucket + 256, 0, 511) for every distance query - key in +-511, the
                                                             bucket as transformers' ``build_relative_position(..., bucket_size=256,
                                                             max_position=512)`` gives it (``rel_bucket``: the bucket itself),
                               ``defect_idx``, ``defects``, ``defects_fp16_only``: see below.
  deberta_v3_ce_hidden.npz, deberta_v3_ce_hidden_510.npz
                               ``hidden_<i>``: the fp64 last hidden state of sequence i (stored as fp32; the 510-token sequence in
                               the second file, to keep every file under 1 MiB).
  deberta_v3_ce_defects_<n>.npz
                               ``<defect>_<k>``: the last hidden states (fp64 arithmetic, stored as fp32) of sequence
                               ``defect_idx[k]`` under six defects an implementation could have, two defects per file --
                                 ``noc2p``     the content-to-position term Q[q] . PK[i] dropped,
                                 ``nop2c``     the position-to-content term K[k] . PQ[i] dropped,
                                 ``mirrored``  both terms read at i(k - q) instead of i(q - k),
                                 ``norelln``   no LayerNorm on the relative embeddings,
                                 ``linear``    the bucket of a distance is the distance itself (clamped), not the log bucket:
                                               differs only beyond 128 tokens, i.e. on the 300-token sequence,
                                 ``scale64``   the content term divided by sqrt(64) instead of sqrt(3 * 64): a defect of 0.08-0.15,
                                               inside 4 e_bf16 -- it is stored for the fp16 test ALONE (``defects_fp16_only``), where
                                               e is ten times smaller.

The GPU test bounds |hidden_hip - hidden_fp64| by 2 e_<type> (the factor the ModernBERT, Gemma and MPNet tests give a second 16-bit
implementation) and wants every defect reference used for that type outside that bound.  An implementation within 2 e of the fp64
states is more than 2 e away from a defect iff the defect is more than 4 e away from them: asserted below for every defect and every
type in which it is used.

    python tests/golden/make_deberta_golden.py
"""
import copy
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "deberta_v3_ce"
VOCAB, PAD, CLS, SEP, FIRST_WORD = 600, 0, 1, 2, 4
LENGTHS = [1, 9, 17, 92, 130, 300, 510]
DEFECT_LENGTHS = [9, 92, 300]
SEED = 43
REL_MEAN, REL_STD = 0.7, 2.0
REL_LN_GAIN = 2.0
QK_SHARPEN = 5.0
LOGIT_SPREAD = 12.0   # the classifier is scaled to this spread of the fp64 logits (the test wants more than 8)
FACTOR = 2.0          # the GPU test's head-room over e_<type>
SPAN, MAX_POS = 256, 512
FP16_ONLY = ["scale64"]


def sequences(rng):
    """[CLS] words [SEP]; from 9 tokens on a pair, [CLS] a [SEP] b [SEP]; a single token is [CLS] alone.  No [PAD] (id 0)."""
    out = []
    for n in LENGTHS:
        s = rng.integers(FIRST_WORD, VOCAB, n).astype(np.int32)
        s[0] = CLS
        if n > 1:
            s[-1] = SEP
        if n >= 9:
            s[n // 3] = SEP
        out.append(s)
    return out


def run(model, ids):
    """-> (last hidden state [n][H], logit) of one sequence."""
    with torch.no_grad():
        t = torch.from_numpy(ids.astype(np.int64))[None]
        out = model(input_ids=t, attention_mask=torch.ones_like(t), output_hidden_states=True)
        return out.hidden_states[-1][0], out.logits[0, 0]


def position_bias(att, query_layer, key_layer, rel_embeddings, scale_factor, c2p=True, p2c=True, mirrored=False, linear=False,
                  content_scale=None):
    """The two position terms of ``DisentangledSelfAttention`` written out for one index i(q, k) -- the form the HIP kernels
    compute -- with switches for the defects.  [batch * heads][q][k]."""
    from transformers.models.deberta_v2.modeling_deberta_v2 import make_log_bucket_position, scaled_size_sqrt

    n, span, heads = query_layer.size(-2), att.pos_ebd_size, att.num_attention_heads
    i = torch.arange(n, dtype=torch.long)
    d = i[:, None] - i[None, :]                      # query - key
    if mirrored:
        d = -d
    b = d if linear else make_log_bucket_position(d, att.position_buckets, att.max_relative_positions).to(torch.long)
    idx = torch.clamp(b + span, 0, 2 * span - 1)     # [q][k]
    rel = rel_embeddings[0:2 * span, :].unsqueeze(0)
    reps = query_layer.size(0) // heads
    pk = att.transpose_for_scores(att.key_proj(rel), heads).repeat(reps, 1, 1)
    pq = att.transpose_for_scores(att.query_proj(rel), heads).repeat(reps, 1, 1)
    scale = scaled_size_sqrt(query_layer, scale_factor).to(query_layer.dtype)
    score = torch.zeros(query_layer.size(0), n, n, dtype=query_layer.dtype)
    if c2p:
        score = score + torch.gather(query_layer @ pk.transpose(-1, -2), -1, idx.expand(query_layer.size(0), n, n)) / scale
    if p2c:   # [k][q] = K[k] . PQ[i(q, k)]
        score = score + torch.gather(key_layer @ pq.transpose(-1, -2), -1, idx.t().expand(query_layer.size(0), n, n)).transpose(-1, -2) / scale
    if content_scale is not None:                   # the content term at another scale: the difference to the model's own
        score = score + (query_layer @ key_layer.transpose(-1, -2)) * (1.0 / content_scale - 1.0 / scale)
    return score


def patched(model, norelln=False, **kw):
    m = copy.deepcopy(model)
    for layer in m.deberta.encoder.layer:
        att = layer.attention.self
        att.disentangled_attention_bias = (lambda q, k, relative_pos, rel_embeddings, scale_factor, att=att:
                                           position_bias(att, q, k, rel_embeddings, scale_factor, **kw))
    if norelln:
        enc = m.deberta.encoder
        enc.get_rel_embedding = lambda: enc.rel_embeddings.weight
    return m


def main():
    from transformers import DebertaV2Config, DebertaV2ForSequenceClassification
    from transformers.models.deberta_v2.modeling_deberta_v2 import build_relative_position

    torch.manual_seed(SEED)
    cfg = DebertaV2Config(vocab_size=VOCAB, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2,
                          max_position_embeddings=MAX_POS, relative_attention=True, position_buckets=SPAN, max_relative_positions=-1,
                          share_att_key=True, pos_att_type=["p2c", "c2p"], norm_rel_ebd="layer_norm", position_biased_input=False,
                          type_vocab_size=0, layer_norm_eps=1e-7, num_labels=1, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0, pooler_dropout=0.0, pooler_hidden_size=256, pooler_hidden_act="gelu",
                          hidden_act="gelu", pad_token_id=PAD)
    model = DebertaV2ForSequenceClassification(cfg).eval().to(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():       # trained-model-like scales: nothing exactly 1 or exactly 0
            if n.endswith("LayerNorm.weight"):
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif n.endswith("LayerNorm.bias"):
                p.copy_(0.05 * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.copy_(0.02 * torch.randn_like(p))
        enc = model.deberta.encoder
        # Embedding(padding_idx=) zeroed this row; trained checkpoints carry ordinary values there
        model.deberta.embeddings.word_embeddings.weight[PAD].copy_(0.02 * torch.randn(cfg.hidden_size))
        enc.rel_embeddings.weight.copy_(REL_MEAN + REL_STD * torch.randn_like(enc.rel_embeddings.weight))
        enc.LayerNorm.weight.mul_(REL_LN_GAIN)
        for layer in enc.layer:
            for lin in (layer.attention.self.query_proj, layer.attention.self.key_proj):
                lin.weight.mul_(QK_SHARPEN)
                lin.bias.mul_(QK_SHARPEN)
        model.classifier.weight.copy_(0.2 * torch.randn_like(model.classifier.weight))
    rng = np.random.default_rng(SEED)
    seqs = sequences(rng)
    assert [len(s) for s in seqs] == LENGTHS and max(LENGTHS) <= MAX_POS
    with torch.no_grad():       # spread the logits around zero: the classifier is linear in its weight
        raw = torch.stack([run(copy.deepcopy(model).double(), s)[1] for s in seqs]) - model.classifier.bias.double()
        gain = LOGIT_SPREAD / float(raw.max() - raw.min())
        model.classifier.weight.mul_(gain)
        model.classifier.bias.copy_(-gain * 0.5 * (raw.max() + raw.min()) + 0.3)

    d = os.path.join(HERE, NAME)
    os.makedirs(d, exist_ok=True)
    model.save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
    with open(os.path.join(d, "config.json")) as f:
        saved = json.load(f)
    assert saved["model_type"] == "deberta-v2" and saved["architectures"] == ["DebertaV2ForSequenceClassification"]
    assert saved["position_buckets"] == SPAN and saved["share_att_key"] is True and saved["type_vocab_size"] == 0
    from safetensors.torch import load_file

    with open(os.path.join(d, "model.safetensors.index.json")) as f:
        shards = sorted(set(json.load(f)["weight_map"].values()))
    names = sorted(set().union(*(load_file(os.path.join(d, s)).keys() for s in shards)))
    assert {"deberta.encoder.rel_embeddings.weight", "deberta.encoder.LayerNorm.weight", "pooler.dense.weight", "classifier.weight"} <= set(names)
    assert not any("position_embeddings" in n or "token_type" in n or "pos_key_proj" in n for n in names)

    m64 = copy.deepcopy(model).double()
    got = [run(m64, s) for s in seqs]
    hidden = [h for h, _ in got]
    logits = np.asarray([float(x) for _, x in got])
    assert logits.max() - logits.min() > 8.0, logits
    e, logits16 = {}, {}
    for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m16 = copy.deepcopy(model).to(dt)          # cast afresh from the fp32 weights
        got16 = [run(m16, s) for s in seqs]
        e[key] = max(float((h16.double() - h).abs().max()) for (h16, _), h in zip(got16, hidden))
        logits16[key] = np.asarray([float(x) for _, x in got16])
    assert all(1e-4 < v < 0.5 for v in e.values()), e

    # the written-out form of the unpatched rule is the model's own: the patching itself changes nothing
    same = patched(m64)
    dev = max(float((run(same, s)[0] - h).abs().max()) for s, h in zip(seqs, hidden))
    assert dev < 1e-9, dev
    defect_models = {
        "noc2p": patched(m64, c2p=False), "nop2c": patched(m64, p2c=False), "mirrored": patched(m64, mirrored=True),
        "norelln": patched(m64, norelln=True), "linear": patched(m64, linear=True), "scale64": patched(m64, content_scale=8.0),
    }
    defect_idx = [LENGTHS.index(n) for n in DEFECT_LENGTHS]
    defects, gaps = {}, {}
    for name, m in defect_models.items():
        per = []
        for k, i in enumerate(defect_idx):
            defects[f"{name}_{k}"] = run(m, seqs[i])[0]
            per.append(float((defects[f"{name}_{k}"] - hidden[i]).abs().max()))
        gaps[name] = max(per)
        for key, v in e.items():
            if key == "bf16" and name in FP16_ONLY:
                continue
            assert gaps[name] > 2 * FACTOR * v, (f"defect '{name}' is only {gaps[name]:.4f} from the fp64 states: inside 2 x the "
                                                 f"test's bound {FACTOR} x e_{key} = {FACTOR * v:.4f}; widen REL_STD / REL_LN_GAIN "
                                                 "(position terms), QK_SHARPEN (scale64)")
    # (the log bucket is the identity up to +-128: the linear defect shows on the 300-token sequence alone)
    assert float((defects["linear_0"] - hidden[defect_idx[0]]).abs().max()) < 1e-9

    rel = build_relative_position(torch.zeros(MAX_POS, 1), torch.zeros(MAX_POS, 1), bucket_size=SPAN, max_position=MAX_POS)[0]
    bucket = torch.cat([rel[0, 1:].flip(0), rel[:, 0]])          # d = -(511) .. -1 (query 0, key -d), then 0 .. 511 (query d, key 0)
    assert bucket.shape == (2 * MAX_POS - 1,) and int(bucket[MAX_POS - 1]) == 0 and int(bucket[MAX_POS]) == 1
    dist_index = torch.clamp(bucket + SPAN, 0, 2 * SPAN - 1)

    np.savez_compressed(os.path.join(HERE, f"{NAME}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(LENGTHS, dtype=np.int32),
                        logits=logits.astype(np.float64), e_bf16=np.float64(e["bf16"]), e_fp16=np.float64(e["fp16"]),
                        logits_bf16=logits16["bf16"], logits_fp16=logits16["fp16"],
                        rel_bucket=bucket.numpy().astype(np.int32), dist_index=dist_index.numpy().astype(np.int32),
                        defect_idx=np.asarray(defect_idx, dtype=np.int32), defects=np.asarray(list(defect_models)),
                        defects_fp16_only=np.asarray(FP16_ONLY))
    small = {f"hidden_{i}": h.numpy().astype(np.float32) for i, h in enumerate(hidden) if LENGTHS[i] != 510}
    np.savez_compressed(os.path.join(HERE, f"{NAME}_hidden.npz"), **small)
    i510 = LENGTHS.index(510)
    np.savez_compressed(os.path.join(HERE, f"{NAME}_hidden_510.npz"), **{f"hidden_{i510}": hidden[i510].numpy().astype(np.float32)})
    order = list(defect_models)
    files = ["expected", "hidden", "hidden_510"]
    for n in range(0, len(order), 2):
        part = {k: v.numpy().astype(np.float32) for k, v in defects.items() if k.rsplit("_", 1)[0] in order[n:n + 2]}
        np.savez_compressed(os.path.join(HERE, f"{NAME}_defects_{n // 2}.npz"), **part)
        files.append(f"defects_{n // 2}")
    for root, _, fs in os.walk(d):
        for fn in fs:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for sfx in files:
        assert os.path.getsize(os.path.join(HERE, f"{NAME}_{sfx}.npz")) < 1 << 20, sfx
    print(NAME, "written: e", e, "defect gaps", gaps, "logits", logits.round(3).tolist(),
          "logit errors", {k: float(np.abs(v - logits).max()) for k, v in logits16.items()},
          "hidden abs max", max(float(h.abs().max()) for h in hidden))


if __name__ == "__main__":
    main()
