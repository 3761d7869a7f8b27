"""Writes the JinaBERT (jina-embeddings-v2) fixtures under tests/golden/ (run on a machine with transformers; CPU, nothing
downloaded).

[UPSTREAM-K] The modelling file (jinaai/jina-bert-implementation, modeling_bert.py) is remote code and not part of transformers: the
tensor names, the config keys and which half of ``mlp.gated_layers`` is activated are written here from knowledge of that module.
The ARITHMETIC is pinned to classes that are installed, piece by piece, and a failed pin stops this script:

  * attention with a bias -- ``BertModel`` (eager attention) adds a float ``attention_mask`` of shape [1][heads][L][L] to the scaled
    scores.  With the position table zeroed and the ALiBi matrix passed as that mask, the fp64 forward restated below (with its
    plain-GELU MLP switch) equals it;
  * the slopes -- ``transformers.models.bloom.modeling_bloom.build_alibi_tensor`` gives the slopes of ``alibi_slopes`` for 4, 6, 8
    and 12 heads;
  * GEGLU -- ``ModernBertMLP.forward`` is ``Wo(act(input) * gate)`` with ``input, gate = Wi(x).chunk(2)``: the restated GEGLU block
    equals it on the same weights (the first half of the columns is the activated one).

  jinabert_l2/                 the checkpoint directory, [UPSTREAM-K] tensor names: hidden 384, 6 heads of 64 (not a power of two: the
                               second branch of the slope rule), intermediate_size 512, 2 layers, vocab 600, type_vocab_size 2,
                               8192 positions.  config.json (model_type "bert", position_embedding_type "alibi", feed_forward_type
                               "geglu", an auto_map), sharded model.safetensors (``pooler.dense.*`` present, as BertModel writes
                               it), modules.json, 1_Pooling/config.json (mean), a word-level tokenizer.json.  The weights are
                               rounded to fp16 before anything is computed and stored as fp16 (every file under 1 MiB), with
                               trained-model-like scales: q / k sharpened (at +-0.02 the attention is uniform and the bias
                               invisible), v / o and MLP gains so that GEGLU leaves GELU's linear range, biases and LayerNorm
                               biases of the order of the activations, token-type row 0 non-zero.
  jinabert_l2_expected.npz     token ids (flat ``ids`` + ``lens``: 1, 9, 17, 92, 130, 300 and 700 tokens) and, in fp64 arithmetic, one
                               sequence per call:
                               ``emb``                 the mean-pooled, L2-normalised last hidden states,
                               ``e_bf16`` / ``e_fp16`` the largest deviation from the fp64 states of the same torch model run in
                                                       that type on the CPU.  That model is ``BertModel``'s embeddings, attention
                                                       and post-LN with each layer's feed-forward swapped for the pinned GEGLU
                                                       block; the ALiBi mask is built in fp32 and handed over in the model's type
                                                       (eager attention adds a mask of its own type only),
                               ``defect_idx``, ``defects``, ``defects_fp16_only``: see below.
  jinabert_l2_defect_<defect>.npz
                               ``<defect>_<k>``: the last hidden states (fp64 arithmetic, stored as fp32, one file per defect) of
                               sequence ``defect_idx[k]`` (9, 92 and 300 tokens) under the defects an implementation could have --
                                 ``nobias``       ALiBi off,
                                 ``signed``       ``key - query`` without the absolute value,
                                 ``prescale``     the bias added before the 1/8 scaling,
                                 ``pow2slopes``   the slopes of 8 heads truncated to 6,
                                 ``headrev``      the slopes in reverse head order,
                                 ``swapglu``      GELU on the second half of ``gated_layers``,
                                 ``notype``       token-type row 0 not added,
                                 ``prenorm``      the LayerNorm in front of each sublayer instead of behind the residual sum,
                                 ``nobias_qkv``   the q / k / v biases dropped.
                               A defect less than 4 e_bf16 from the fp64 states is listed in ``defects_fp16_only``.
  jinabert_l2_hidden.npz, jinabert_l2_hidden_700.npz
                               ``hidden_<i>``: the fp64 last hidden state of sequence i (stored as fp32; the 700-token sequence in
                               the second file, to keep every file under 1 MiB).

The GPU test bounds |hidden_hip - hidden_fp64| by 2 e_<type> (DESIGN.md 4.8's factor for a second 16-bit implementation) and wants
every defect reference outside that bound.  An implementation within 2 e of the fp64 states is more than 2 e away from a defect iff
the defect is more than 4 e away from them: asserted below for every defect used for a type.

    python tests/golden/make_jinabert_golden.py
"""
import copy
import json
import math
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
NAME = "jinabert_l2"
VOCAB, PAD, UNK, CLS, SEP, FIRST_WORD = 600, 0, 1, 2, 3, 4
LENGTHS = [1, 9, 17, 92, 130, 300, 700]
DEFECT_LENGTHS = [9, 92, 300]
SEED = 71
QK_SHARPEN = 5.0
VO_GAIN = 3.0         # value and attention.output.dense: an attention sublayer of the order of the residual stream
TYPE_STD = 0.05       # token-type rows: of the order of the word embeddings
BIAS_STD = 0.3        # projection biases: of the order of the projections' outputs
LN_BIAS_STD = 0.1
MLP_GAIN = (3.0, 2.0)  # gated_layers, and wo: a gate that leaves GELU's linear range
FACTOR = 2.0          # the GPU test's head-room over e_<type>
HIDDEN, HEADS, FFN, LAYERS, MAX_POS, EPS = 384, 6, 512, 2, 8192, 1e-12
DEFECTS = ["nobias", "signed", "prescale", "pow2slopes", "headrev", "swapglu", "notype", "prenorm", "nobias_qkv"]
FP16_ONLY = []


def sequences(rng):
    out = []
    for n in LENGTHS:
        s = rng.integers(FIRST_WORD, VOCAB, n).astype(np.int32)
        s[0] = CLS
        if n > 1:
            s[-1] = SEP
        out.append(s)
    return out


def write_tokenizer(path):
    """Word-level tokenizer: [PAD] 0, [UNK] 1, [CLS] 2, [SEP] 3, then the words w0 .. w595."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {"[PAD]": PAD, "[UNK]": UNK, "[CLS]": CLS, "[SEP]": SEP}
    vocab.update({f"w{i}": FIRST_WORD + i for i in range(VOCAB - FIRST_WORD)})
    tk = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]",
                                                      special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    tk.save(path)


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def slopes_of(heads, defect=None):
    from tensor_truth_amd.jinabert import alibi_slopes

    if defect == "pow2slopes":
        return alibi_slopes(8)[:heads]
    s = alibi_slopes(heads)
    return s[::-1] if defect == "headrev" else s


def alibi_matrix(n, heads, dtype=torch.float64, defect=None):
    """[heads][n][n]: -slope_h |i - j| (what is added to the scaled scores)."""
    i = torch.arange(n, dtype=dtype)
    dist = i[None, :] - i[:, None]                 # key - query
    if defect != "signed":
        dist = dist.abs()
    return -torch.tensor(slopes_of(heads, defect), dtype=dtype)[:, None, None] * dist[None]


def forward64(sd, ids, mlp="geglu", defect=None):
    """The model restated in fp64 on the state dict ``sd`` ([UPSTREAM-K] names; ``mlp`` "gelu": BERT's own feed-forward, names
    ``intermediate.dense`` / ``output.dense`` / ``output.LayerNorm`` -- the switch the BertModel pin uses), one defect on."""
    n = len(ids)
    lin = lambda x, name: x @ sd[name + ".weight"].T + (sd[name + ".bias"] if name + ".bias" in sd else 0.0)  # noqa: E731
    ln = lambda x, name: layer_norm(x, sd[name + ".weight"], sd[name + ".bias"], EPS)  # noqa: E731
    x = sd["embeddings.word_embeddings.weight"][torch.from_numpy(ids.astype(np.int64))]
    if defect != "notype":
        x = x + sd["embeddings.token_type_embeddings.weight"][0]
    x = ln(x, "embeddings.LayerNorm")
    bias = alibi_matrix(n, HEADS, defect=defect)

    def attention(h, p):
        q, k, v = (lin(h, p + f"attention.self.{m}") for m in ("query", "key", "value"))
        if defect == "nobias_qkv":
            q, k, v = (h @ sd[p + f"attention.self.{m}.weight"].T for m in ("query", "key", "value"))
        q, k, v = (t.view(n, HEADS, 64) for t in (q, k, v))
        s = torch.einsum("qhd,khd->hqk", q, k)
        if defect == "nobias":
            s = s / math.sqrt(64)
        elif defect == "prescale":
            s = (s + bias) / math.sqrt(64)
        else:
            s = s / math.sqrt(64) + bias
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, HIDDEN)
        return lin(a, p + "attention.output.dense")

    def feed_forward(h, p):
        if mlp == "gelu":
            return lin(torch.nn.functional.gelu(lin(h, p + "intermediate.dense")), p + "output.dense")
        g = lin(h, p + "mlp.gated_layers")
        a, m = g[:, :FFN], g[:, FFN:]
        if defect == "swapglu":
            a, m = m, a
        return lin(torch.nn.functional.gelu(a) * m, p + "mlp.wo")

    for i in range(LAYERS):
        p = f"encoder.layer.{i}."
        ln1 = lambda t: ln(t, p + "attention.output.LayerNorm")  # noqa: E731
        ln2 = lambda t: ln(t, p + ("output.LayerNorm" if mlp == "gelu" else "mlp.layernorm"))  # noqa: E731
        if defect == "prenorm":
            x = x + attention(ln1(x), p)
            x = x + feed_forward(ln2(x), p)
        else:
            x = ln1(x + attention(x, p))
            x = ln2(x + feed_forward(x, p))
    return x


class GegluIntermediate(torch.nn.Module):
    """What replaces ``BertIntermediate`` in the reference model: ``act(input) * gate`` of ``ModernBertMLP`` (pinned below);
    ``BertOutput`` behind it is wo + the residual LayerNorm."""

    def __init__(self):
        super().__init__()
        self.gated_layers = torch.nn.Linear(HIDDEN, 2 * FFN, bias=False)
        self.act = torch.nn.GELU()

    def forward(self, x):
        a, g = self.gated_layers(x).chunk(2, dim=-1)
        return self.act(a) * g


def hidden_of(model, ids, dt):
    n = len(ids)
    mask = alibi_matrix(n, HEADS, dtype=torch.float64 if dt == torch.float64 else torch.float32).to(dt)[None]
    with torch.no_grad():
        return model(input_ids=torch.from_numpy(ids.astype(np.int64))[None], attention_mask=mask).last_hidden_state[0]


def upstream_names(sd):
    """The reference model's state dict under the [UPSTREAM-K] names: the swapped feed-forward is ``mlp.gated_layers`` / ``mlp.wo`` /
    ``mlp.layernorm``; the (zeroed) position table is not part of a JinaBERT checkpoint."""
    out = {}
    for k, v in sd.items():
        if k == "embeddings.position_embeddings.weight":
            continue
        k = re.sub(r"(layer\.\d+\.)intermediate\.gated_layers", r"\1mlp.gated_layers", k)
        k = re.sub(r"(layer\.\d+\.)output\.dense", r"\1mlp.wo", k)
        k = re.sub(r"(layer\.\d+\.)output\.LayerNorm", r"\1mlp.layernorm", k)
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
                   "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}, f, indent=2)


def pin_slopes():
    from transformers.models.bloom.modeling_bloom import build_alibi_tensor

    from tensor_truth_amd.jinabert import alibi_slopes

    for heads in (4, 6, 8, 12):
        bloom = build_alibi_tensor(torch.ones(1, 3), heads, torch.float32)[:, 0, 1].double()      # slope * position 1
        ours = torch.tensor(alibi_slopes(heads), dtype=torch.float64)
        assert bloom.shape == ours.shape and float(((bloom - ours) / ours).abs().max()) < 1e-6, (heads, bloom, ours)
    assert alibi_slopes(8) == [2.0 ** -(i + 1) for i in range(8)]


def pin_geglu(sd64):
    """The restated GEGLU block (without the residual LayerNorm) equals ModernBertMLP on layer 0's weights."""
    from transformers import ModernBertConfig
    from transformers.models.modernbert.modeling_modernbert import ModernBertMLP

    mlp = ModernBertMLP(ModernBertConfig(hidden_size=HIDDEN, intermediate_size=FFN, mlp_bias=True, hidden_activation="gelu",
                                         mlp_dropout=0.0)).eval().double()
    p = "encoder.layer.0.mlp."
    with torch.no_grad():
        mlp.Wi.weight.copy_(sd64[p + "gated_layers.weight"])
        mlp.Wi.bias.zero_()
        mlp.Wo.weight.copy_(sd64[p + "wo.weight"])
        mlp.Wo.bias.copy_(sd64[p + "wo.bias"])
        x = torch.randn(37, HIDDEN, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        g = x @ sd64[p + "gated_layers.weight"].T
        ours = (torch.nn.functional.gelu(g[:, :FFN]) * g[:, FFN:]) @ sd64[p + "wo.weight"].T + sd64[p + "wo.bias"]
        err = float((mlp(x) - ours).abs().max())
    assert err < 1e-12, err
    return err


def main():
    from transformers import BertConfig, BertModel

    pin_slopes()
    torch.manual_seed(SEED)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=FFN, num_hidden_layers=LAYERS,
                     type_vocab_size=2, max_position_embeddings=MAX_POS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                     layer_norm_eps=EPS, hidden_act="gelu", pad_token_id=PAD)
    cfg._attn_implementation = "eager"
    bert = BertModel(cfg, add_pooling_layer=True).eval().to(torch.float32)
    assert cfg._attn_implementation == "eager"
    with torch.no_grad():
        for n, p in bert.named_parameters():        # trained-model-like scales: nothing exactly 1 or exactly 0
            if "LayerNorm.weight" in n:
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif "LayerNorm.bias" in n:
                p.copy_(LN_BIAS_STD * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.copy_(BIAS_STD * torch.randn_like(p))
        emb = bert.embeddings
        emb.position_embeddings.weight.zero_()      # no position table
        emb.word_embeddings.weight[PAD].copy_(0.02 * torch.randn(HIDDEN))       # Embedding(padding_idx=) zeroed this row
        emb.token_type_embeddings.weight.copy_(TYPE_STD * torch.randn_like(emb.token_type_embeddings.weight))
        for layer in bert.encoder.layer:
            att = layer.attention
            for lin in (att.self.query, att.self.key):
                lin.weight.mul_(QK_SHARPEN)
            for lin in (att.self.value, att.output.dense):
                lin.weight.mul_(VO_GAIN)
            layer.intermediate.dense.weight.mul_(MLP_GAIN[0])
            layer.output.dense.weight.mul_(MLP_GAIN[1])
    rng = np.random.default_rng(SEED)
    seqs = sequences(rng)
    assert [len(s) for s in seqs] == LENGTHS and max(LENGTHS) <= MAX_POS

    # pin 1: BertModel (plain GELU feed-forward, zeroed position table, ALiBi as the 4-D mask) == the restated forward, mlp="gelu"
    b64 = copy.deepcopy(bert).double()
    sdb = {k: v.double() for k, v in bert.state_dict().items()}
    pin_bert = max(float((forward64(sdb, s, mlp="gelu") - hidden_of(b64, s, torch.float64)).abs().max()) for s in seqs[:5])
    assert pin_bert < 1e-11, pin_bert
    # the mask is not ignored: without it the model is the `nobias` defect, far away
    with torch.no_grad():
        plain = b64(input_ids=torch.from_numpy(seqs[3].astype(np.int64))[None]).last_hidden_state[0]
    assert float((plain - forward64(sdb, seqs[3], mlp="gelu", defect="nobias")).abs().max()) < 1e-11
    assert float((plain - hidden_of(b64, seqs[3], torch.float64)).abs().max()) > 1e-2

    # the reference model: the same embeddings, attention and post-LN, each layer's feed-forward swapped for the GEGLU block
    model = copy.deepcopy(bert)
    with torch.no_grad():
        for layer in model.encoder.layer:
            layer.intermediate = GegluIntermediate()
            layer.intermediate.gated_layers.weight.normal_(0.0, 0.02).mul_(MLP_GAIN[0])
        model = model.half().float()                # the stored weights ARE the model's: fp16 values
    stored = {k: v.half() for k, v in upstream_names(model.state_dict()).items()}
    assert "embeddings.position_embeddings.weight" not in stored and "pooler.dense.weight" in stored
    assert stored["encoder.layer.1.mlp.gated_layers.weight"].shape == (2 * FFN, HIDDEN) and "encoder.layer.1.mlp.gated_layers.bias" not in stored
    assert {"encoder.layer.0.attention.output.dense.bias", "encoder.layer.0.attention.output.LayerNorm.weight", "encoder.layer.0.mlp.wo.bias",
            "encoder.layer.0.mlp.layernorm.bias", "encoder.layer.0.attention.self.key.bias"} <= set(stored)
    sd64 = {k: v.double() for k, v in stored.items()}
    pin_mlp = pin_geglu(sd64)

    m64 = copy.deepcopy(model).double()
    hidden = [hidden_of(m64, s, torch.float64) for s in seqs]
    restated = max(float((forward64(sd64, s) - h).abs().max()) for s, h in zip(seqs, hidden))
    assert restated < 1e-9, restated
    embv = np.stack([torch.nn.functional.normalize(h.mean(0), dim=0).numpy() for h in hidden])
    e = {}
    for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m16 = copy.deepcopy(model).to(dt)           # cast afresh from the stored weights
        e[key] = max(float((hidden_of(m16, s, dt).double() - h).abs().max()) for s, h in zip(seqs, hidden))
    assert all(1e-4 < v < 0.5 for v in e.values()), e

    defect_idx = [LENGTHS.index(n) for n in DEFECT_LENGTHS]
    defects, gaps = {}, {}
    for dn in DEFECTS:
        for k, i in enumerate(defect_idx):
            defects[f"{dn}_{k}"] = forward64(sd64, seqs[i], defect=dn)
        gaps[dn] = max(float((defects[f"{dn}_{k}"] - hidden[i]).abs().max()) for k, i in enumerate(defect_idx))
        for key, v in e.items():
            if key == "bf16" and dn in FP16_ONLY:
                continue
            assert gaps[dn] > 2 * FACTOR * v, (f"defect '{dn}' is only {gaps[dn]:.4f} from the fp64 states: inside 2 x the test's bound "
                                               f"{FACTOR} x e_{key} = {FACTOR * v:.4f}; rescale the weights or list it in FP16_ONLY")

    d = os.path.join(HERE, NAME)
    os.makedirs(d, exist_ok=True)
    for fn in os.listdir(d):                        # (a re-run with another shard count leaves no stale shard behind)
        if fn.endswith(".safetensors"):
            os.remove(os.path.join(d, fn))
    write_sharded(d, stored)
    sentence_transformers_files(d)
    write_tokenizer(os.path.join(d, "tokenizer.json"))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"architectures": ["JinaBertModel"], "model_type": "bert", "position_embedding_type": "alibi",
                   "feed_forward_type": "geglu", "hidden_act": "gelu", "hidden_size": HIDDEN, "num_hidden_layers": LAYERS,
                   "num_attention_heads": HEADS, "intermediate_size": FFN, "vocab_size": VOCAB, "type_vocab_size": 2,
                   "layer_norm_eps": EPS, "max_position_embeddings": MAX_POS, "pad_token_id": PAD, "hidden_dropout_prob": 0.0,
                   "attention_probs_dropout_prob": 0.0, "initializer_range": 0.02, "emb_pooler": "mean", "torch_dtype": "float16",
                   "auto_map": {"AutoConfig": "jinaai/jina-bert-implementation--configuration_bert.JinaBertConfig",
                                "AutoModel": "jinaai/jina-bert-implementation--modeling_bert.JinaBertModel"}}, f, indent=2)

    out = os.path.join(HERE, NAME)
    np.savez_compressed(out + "_expected.npz", ids=np.concatenate(seqs), lens=np.asarray(LENGTHS, dtype=np.int32),
                        emb=embv.astype(np.float64), e_bf16=np.float64(e["bf16"]), e_fp16=np.float64(e["fp16"]),
                        defect_idx=np.asarray(defect_idx, dtype=np.int32), defects=np.asarray(DEFECTS),
                        defects_fp16_only=np.asarray(FP16_ONLY, dtype="<U16"))
    for dn in DEFECTS:
        np.savez_compressed(out + f"_defect_{dn}.npz",
                            **{f"{dn}_{k}": defects[f"{dn}_{k}"].numpy().astype(np.float32) for k in range(len(defect_idx))})
    i700 = LENGTHS.index(700)
    np.savez_compressed(out + "_hidden.npz", **{f"hidden_{i}": h.numpy().astype(np.float32) for i, h in enumerate(hidden) if i != i700})
    np.savez_compressed(out + "_hidden_700.npz", **{f"hidden_{i700}": hidden[i700].numpy().astype(np.float32)})
    for root, _, files in os.walk(d):
        for fn in files:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for fn in os.listdir(HERE):
        if fn.startswith(NAME + "_") and fn.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn
    print(NAME, "written: pins: BertModel", pin_bert, "ModernBertMLP", pin_mlp, "restated", restated, "; e", e, "; defect gaps", gaps,
          "; hidden abs max", max(float(h.abs().max()) for h in hidden))


if __name__ == "__main__":
    main()
