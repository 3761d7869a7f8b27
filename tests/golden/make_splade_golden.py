"""Writes the SPLADE fixtures under tests/golden/ (run on a machine with transformers; CPU, nothing downloaded).

[UPSTREAM-K] A SPLADE checkpoint is a ``BertForMaskedLM``; a text's weight for vocabulary id v is ``max_t log1p(relu(logit[t][v]))``
over every token of the text, ``[CLS]`` and ``[SEP]`` included (sentence-transformers' ``SpladePooling`` with ``pooling_strategy``
"max" and ``activation_function`` "relu", multiplied by the attention mask; naver's ``Splade`` model likewise), and a pair's score is
the dot product of the two weight vectors -- written here from knowledge of those projects, which are not installed.  The model's
arithmetic IS pinned to a class that is installed, and a failed pin stops the script: ``BertForMaskedLM`` (eager attention) equals
the fp64 forward restated below, logits included, on every text.

  splade_l2/                config.json (model_type bert: 2 layers, hidden 128, 2 heads of 64, ffn 256, 66 positions, vocabulary 600 --
                            640 after the loader's padding to a multiple of 128, so 40 padding ids), model.safetensors
                            (BertForMaskedLM's names, ``bert.`` prefix, pooler-free; the decoder is TIED: no
                            ``cls.predictions.decoder.weight``) and a word-level tokenizer.json ([PAD] [UNK] [CLS] [SEP] [MASK] at
                            0 .. 4, then w0 .. w594).  The weights are rounded to fp16 before anything is computed.  The model is
                            LEXICAL, as a trained one is (main()): a token activates its own id and the 7 ids of its cluster, and
                            the decoder bias (mean -6) keeps everything else off -- a text activates 2 to 25 % of the vocabulary.
  splade_l2_expected.npz    the token ids (with [CLS] and [SEP]) and the texts of 4 queries and 24 passages: passage i belongs to
                            query i // 6 and holds the first 6/6 .. 1/6 of its words, then filler words; one passage is a single
                            word (3 tokens), one fills the 64-token limit exactly, one is longer and truncated.  In fp64
                            arithmetic: ``pre`` [28][600] (max over the tokens of the logits), ``weights`` [28][600]
                            (log1p(relu(pre))), ``lex`` [4][24]; ``e_<quantity>_<type>`` for pre, weights, lex and the types
                            bf16, fp16: the largest deviation from fp64 of the same torch modules (BertForMaskedLM, amax, relu,
                            log1p) run in that type on the CPU, the scores evaluated in fp64 ON those vectors; ``prune8_<type>``
                            [28]: the texts whose 8th and 9th largest weights are more than 4 e_weights_<type> apart (whose 8
                            largest weights an implementation within 2 e must therefore agree on; at least one text per type); ``max_length`` 64.
  splade_l2_defect_<d>.npz  ``weights`` and ``lex`` in fp64 arithmetic (stored as fp32) under the defects an implementation could have:
                              ``sum``           the tokens' weights summed instead of maximised,
                              ``nolog``         relu only,
                              ``norelu``        negative maxima kept,
                              ``nobias``        the decoder bias not added,
                              ``notransform``   the decoder applied to the raw hidden state (no dense, GELU, LayerNorm),
                              ``skipspecials``  the [CLS] and [SEP] rows left out of the maximum.

The GPU test bounds |hip - fp64| by 2 e_<type> (DESIGN.md 4.8's factor for a second 16-bit implementation) and wants every defect
outside that bound, which holds iff the defect is more than 4 e from fp64 -- asserted below for ``weights`` and ``lex`` and both types.
Also asserted: in every text at most 5 % of the ids have an fp64 pre-activation within 2 e_pre of the coarser type of zero (the band
inside which the test lets an id be kept or not); every text keeps at least 8 ids; for every query, consecutive fp64 ``lex`` scores
among its top 6 differ by more than 4 e of the coarser type, so the tests can demand the fp64 order.

    python tests/golden/make_splade_golden.py
"""
import copy
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
NAME = "splade_l2"
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
PAD, UNK, CLS, SEP, MASK = range(5)
FIRST_WORD = len(SPECIALS)
VOCAB = 600
HIDDEN, HEADS, FFN, LAYERS, MAX_POS, EPS = 128, 2, 256, 2, 66, 1e-12
MAX_LEN = 64
QUERY_BODIES = [6, 7, 9, 8]
# passage i belongs to query i // 6 and holds the first TAKE(i % 6) of its words, then DOC_EXTRA[i] filler words no query holds
DOC_EXTRA = [3, 9, 16, 24, 33, 0, 4, 14, 23, 41, 59, 1, 2, 8, 26, 45, 64, 0, 0, 5, 12, 22, 30, 56]
SEED = 3
EMB_STD, HEAD_DENSE_STD, BIAS_STD, LN_BIAS_STD = 0.12, 0.05, 0.1, 0.03
CLUSTER, CLUSTER_RHO, POS_STD, RESIDUAL_GAIN, TOP_BOOST = 8, 0.84, 0.02, 0.3, 3.0
DEC_BIAS_MEAN, DEC_BIAS_STD = -6.0, 0.5
FACTOR = 2.0
BAND_SHARE = 0.05
DEFECTS = ["sum", "nolog", "norelu", "nobias", "notransform", "skipspecials"]
QUANTITIES = ["pre", "weights", "lex"]


def layout(body):
    """[CLS] body [SEP], cut to the limit keeping the closing token (what the tokenizer call does)."""
    ids = [CLS] + [int(t) for t in body] + [SEP]
    return ids if len(ids) <= MAX_LEN else ids[: MAX_LEN - 1] + [SEP]


def take_count(n_words, k):
    return max(1, (n_words * (6 - k) + 5) // 6)


def bodies(rng):
    """-> (query bodies, passage bodies).  The vocabulary comes in clusters of CLUSTER ids that activate one another (main()); every
    query word is drawn from a cluster of its own and the filler words from clusters no query word lives in, so a passage's score
    is graded by the number of query words it holds and the filler adds little."""
    clusters = rng.permutation(np.arange(1, VOCAB // CLUSTER))        # (cluster 0 holds the special tokens)
    n_qw = sum(QUERY_BODIES)
    qwords = np.asarray([CLUSTER * c + rng.integers(0, CLUSTER) for c in clusters[:n_qw]], dtype=np.int32)
    filler = np.concatenate([np.arange(CLUSTER * c, CLUSTER * (c + 1)) for c in clusters[n_qw:]]).astype(np.int32)
    qs, at = [], 0
    for n in QUERY_BODIES:
        qs.append(qwords[at:at + n].copy())
        at += n
    ds = []
    for i, extra in enumerate(DOC_EXTRA):
        take = qs[i // 6][: take_count(len(qs[i // 6]), i % 6)]
        pool = rng.choice(filler, max(2, extra // 3))
        ds.append(np.concatenate([take, rng.choice(pool, extra)]).astype(np.int32))
    ds[17] = ds[17][:1]                                   # a single word: 3 tokens
    return qs, ds


def write_tokenizer(path):
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {t: i for i, t in enumerate(SPECIALS)}
    vocab.update({f"w{i}": FIRST_WORD + i for i in range(VOCAB - FIRST_WORD)})
    assert len(vocab) == VOCAB
    tk = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tk.add_special_tokens(SPECIALS)
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]",
                                                      special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    tk.save(path)


def text_of(body):
    return " ".join(f"w{int(t) - FIRST_WORD}" for t in body)


# ---- the model, restated in fp64 ---------------------------------------------------------------------------------------------------
def layer_norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def forward64(sd, ids):
    """-> the last hidden state [n][H] of BertModel (names under ``bert.``)."""
    n = len(ids)
    lin = lambda x, name: x @ sd[name + ".weight"].T + sd[name + ".bias"]  # noqa: E731
    ln = lambda x, name: layer_norm(x, sd[name + ".weight"], sd[name + ".bias"])  # noqa: E731
    e = "bert.embeddings."
    x = (sd[e + "word_embeddings.weight"][torch.as_tensor(np.asarray(ids, dtype=np.int64))] + sd[e + "position_embeddings.weight"][:n]
         + sd[e + "token_type_embeddings.weight"][0])
    x = ln(x, e + "LayerNorm")
    dh = HIDDEN // HEADS
    for i in range(LAYERS):
        p = f"bert.encoder.layer.{i}."
        q, k, v = (lin(x, p + f"attention.self.{m}").view(n, HEADS, dh) for m in ("query", "key", "value"))
        s = torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(dh)
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, HIDDEN)
        x = ln(x + lin(a, p + "attention.output.dense"), p + "attention.output.LayerNorm")
        f = lin(gelu(lin(x, p + "intermediate.dense")), p + "output.dense")
        x = ln(x + f, p + "output.LayerNorm")
    return x


def logits64(sd, h, defect=None):
    """The masked-language-model head on hidden states [n][H] -> logits [n][VOCAB] (tied decoder)."""
    c = "cls.predictions."
    t = h
    if defect != "notransform":
        t = layer_norm(gelu(h @ sd[c + "transform.dense.weight"].T + sd[c + "transform.dense.bias"]),
                       sd[c + "transform.LayerNorm.weight"], sd[c + "transform.LayerNorm.bias"])
    out = t @ sd["bert.embeddings.word_embeddings.weight"].T
    return out if defect == "nobias" else out + sd[c + "bias"]


def weights_of(logits, defect=None):
    """Logits [n][VOCAB] of one text -> (pre [VOCAB], weights [VOCAB])."""
    if defect == "skipspecials":
        logits = logits[1:-1]
    pre = logits.max(0).values
    if defect == "sum":
        return pre, torch.log1p(torch.relu(logits)).sum(0)
    if defect == "nolog":
        return pre, torch.relu(pre)
    if defect == "norelu":
        return pre, torch.where(pre < 0, pre, torch.log1p(torch.relu(pre)))
    return pre, torch.log1p(torch.relu(pre))


def reference(sd, hiddens, n_q, defect=None):
    got = [weights_of(logits64(sd, h, defect), defect) for h in hiddens]
    pre = np.stack([p.numpy() for p, _ in got])
    w = np.stack([x.numpy() for _, x in got])
    return pre, w, w[:n_q] @ w[n_q:].T


def model_logits(model, ids):
    with torch.no_grad():
        return model(input_ids=torch.as_tensor(np.asarray(ids, dtype=np.int64))[None]).logits[0]


def top_gap(rows):
    return min(float(np.min(-np.diff(np.sort(r)[::-1][:6]))) for r in rows)


def main():
    from safetensors.torch import save_file
    from transformers import BertConfig, BertForMaskedLM

    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    qs, ds = bodies(rng)
    n_q = len(qs)
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=FFN, num_hidden_layers=LAYERS,
                     type_vocab_size=2, max_position_embeddings=MAX_POS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                     layer_norm_eps=EPS, hidden_act="gelu", pad_token_id=PAD, tie_word_embeddings=True)
    cfg._attn_implementation = "eager"
    model = BertForMaskedLM(cfg).eval().to(torch.float32)
    assert cfg._attn_implementation == "eager"
    with torch.no_grad():
        # a LEXICAL model, as a trained masked-language model is: the residual stream keeps a token's own embedding (small
        # attention / FFN outputs, a small position table), the head's dense layer is close to the identity, and the word
        # embeddings come in clusters of CLUSTER correlated words -- so that, through the tied decoder, a token activates its own id
        # and its cluster's (expansion) and little else
        centers = torch.randn((VOCAB + CLUSTER - 1) // CLUSTER, HIDDEN)
        for n, p in model.named_parameters():        # trained-model-like scales: nothing exactly 1 or exactly 0
            if "LayerNorm.weight" in n:
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif "LayerNorm.bias" in n:
                p.copy_(LN_BIAS_STD * torch.randn_like(p))
            elif n == "cls.predictions.bias":
                p.copy_(DEC_BIAS_MEAN + DEC_BIAS_STD * torch.randn_like(p))
                # eight ids weigh clearly more, as frequent terms do in a trained model: [CLS], [SEP] and the six words of query 0 --
                # the texts that hold exactly these on top have a clear cut behind their 8th weight (``prune8``)
                p[torch.as_tensor([CLS, SEP] + [int(t) for t in qs[0]])] += TOP_BOOST
            elif n.endswith(".bias"):
                p.copy_(BIAS_STD * torch.randn_like(p))
            elif "word_embeddings" in n:
                own = torch.randn_like(p)
                p.copy_(EMB_STD * (CLUSTER_RHO * centers[torch.arange(VOCAB) // CLUSTER] + math.sqrt(1 - CLUSTER_RHO ** 2) * own))
            elif "position_embeddings" in n or "token_type_embeddings" in n:
                p.copy_(POS_STD * torch.randn_like(p))
            elif "transform.dense.weight" in n:
                p.copy_(torch.eye(HIDDEN) + HEAD_DENSE_STD * torch.randn_like(p))
            elif n.endswith(".weight") and p.dim() == 2:
                gain = RESIDUAL_GAIN if n.endswith("output.dense.weight") else 1.0
                p.copy_(gain * torch.randn_like(p) / math.sqrt(p.shape[1]))
        model = model.half().float()                 # the stored weights ARE the model's: fp16 values
    assert model.cls.predictions.decoder.weight.data_ptr() == model.bert.embeddings.word_embeddings.weight.data_ptr(), "not tied"
    stored = {k: v.half().contiguous() for k, v in model.state_dict().items()
              if k not in ("bert.embeddings.position_ids", "cls.predictions.decoder.weight", "cls.predictions.decoder.bias")}
    assert "cls.predictions.bias" in stored and not any(k.startswith("bert.pooler") for k in stored)
    sd64 = {k: v.double() for k, v in stored.items()}

    seqs = [layout(b) for b in qs + ds]
    lens = [len(s) for s in seqs]
    assert min(lens) == 3 and max(lens) == MAX_LEN and sum(len(b) + 2 > MAX_LEN for b in ds) == 1 \
        and sum(len(b) + 2 == MAX_LEN for b in ds) == 1, lens
    hiddens = [forward64(sd64, ids) for ids in seqs]

    # pin: BertForMaskedLM == the forward and the head restated above
    m64 = copy.deepcopy(model).double()
    pin = max(float((model_logits(m64, ids) - logits64(sd64, h)).abs().max()) for ids, h in zip(seqs, hiddens))
    assert pin < 1e-10, pin

    pre, weights, lex = reference(sd64, hiddens, n_q)
    active = (pre > 0).mean(1)

    e = {q: {} for q in QUANTITIES}
    for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m16 = copy.deepcopy(model).to(dt)             # cast afresh from the stored weights
        lg = [model_logits(m16, ids) for ids in seqs]
        p16 = np.stack([x.amax(0).double().numpy() for x in lg])
        w16 = np.stack([torch.log1p(torch.relu(x.amax(0))).double().numpy() for x in lg])
        for q, a, r in zip(QUANTITIES, (p16, w16, w16[:n_q] @ w16[n_q:].T), (pre, weights, lex)):
            e[q][key] = float(np.abs(a - r).max())
    coarse = {q: max(e[q].values()) for q in QUANTITIES}
    failed = []
    band = (np.abs(pre) <= FACTOR * coarse["pre"]).mean(1)
    if not band.max() <= BAND_SHARE:
        failed.append(f"the band |pre| <= 2 e_pre = {FACTOR * coarse['pre']:.4f} holds {band.max():.3%} of a text's ids (limit 5 %)")
    kept = (weights > 0).sum(1)
    if not kept.min() >= 8:
        failed.append(f"a text keeps only {kept.min()} ids")
    gap = top_gap(lex)
    if not gap > 2 * FACTOR * coarse["lex"]:
        failed.append(f"top-6 lex scores only {gap:.5f} apart: 4 e = {2 * FACTOR * coarse['lex']:.5f}")
    srt = np.sort(weights, 1)[:, ::-1]
    prune8 = {t: (srt[:, 7] - srt[:, 8]) > 2 * FACTOR * e["weights"][t] for t in e["weights"]}
    for t, ok in prune8.items():
        if not ok.any():
            failed.append(f"too few texts whose 8th and 9th weights stand 4 e_{t} apart: {ok.astype(int).tolist()}")

    defects, dgaps = {}, {}
    for dn in DEFECTS:
        _, dw, dl = reference(sd64, hiddens, n_q, defect=dn)
        defects[dn] = {"weights": dw, "lex": dl}
        for q, a, r in (("weights", dw, weights), ("lex", dl, lex)):
            dgaps[f"{dn}:{q}"] = g = float(np.abs(a - r).max())
            if not g > 2 * FACTOR * coarse[q]:
                failed.append(f"defect {dn}:{q} is only {g:.5f} from fp64: inside 4 e = {2 * FACTOR * coarse[q]:.5f}")
    summary = dict(seed=SEED, pin=pin, e=e, active_mean=float(active.mean()), active_max=float(active.max()), band_mean=float(band.mean()),
                   band_max=float(band.max()), kept_min=int(kept.min()), kept_max=int(kept.max()), lex_gap=gap, prune8={t: int(v.sum()) for t, v in prune8.items()},
                   dgaps=dgaps, lex_range=(float(lex.min()), float(lex.max())))
    if os.environ.get("SPLADE_GOLDEN_PROBE"):
        print("PROBE", "ok" if not failed else "FAILED", json.dumps(summary), failed)
        return
    assert not failed, (failed, summary)

    # ---- write ------------------------------------------------------------------------------------------------------------------
    d = os.path.join(HERE, NAME)
    os.makedirs(d, exist_ok=True)
    save_file(stored, os.path.join(d, "model.safetensors"), metadata={"format": "pt"})
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"architectures": ["BertForMaskedLM"], "model_type": "bert", "hidden_size": HIDDEN, "num_hidden_layers": LAYERS,
                   "num_attention_heads": HEADS, "intermediate_size": FFN, "vocab_size": VOCAB, "type_vocab_size": 2,
                   "layer_norm_eps": EPS, "max_position_embeddings": MAX_POS, "pad_token_id": PAD, "hidden_act": "gelu",
                   "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0, "initializer_range": 0.02,
                   "position_embedding_type": "absolute", "tie_word_embeddings": True, "torch_dtype": "float16"}, f, indent=2)
    write_tokenizer(os.path.join(d, "tokenizer.json"))

    # the package's loader reads back what is restated here
    from tensor_truth_amd import splade as ts

    lcfg, bert, head, tk, _ = ts.load_checkpoint(d)
    assert (lcfg.vocab_size, lcfg.hidden, lcfg.layers, lcfg.max_pos) == (VOCAB, HIDDEN, LAYERS, MAX_POS)
    assert torch.equal(head["decoder.weight"].double(), sd64["bert.embeddings.word_embeddings.weight"])
    assert torch.equal(head["bias"].double(), sd64["cls.predictions.bias"])
    texts = [text_of(b) for b in qs + ds]
    assert [tk.encode(t, MAX_LEN) for t in texts] == seqs, "the tokenizer's ids are not the layout restated here"

    out = os.path.join(HERE, NAME)
    np.savez_compressed(out + "_expected.npz", ids=np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]),
                        lens=np.asarray(lens, dtype=np.int32), n_queries=np.int32(n_q), texts=np.asarray(texts),
                        max_length=np.int32(MAX_LEN), pre=pre, weights=weights, lex=lex, defects=np.asarray(DEFECTS),
                        **{f"prune8_{t}": v for t, v in prune8.items()},
                        **{f"e_{q}_{t}": np.float64(v) for q in QUANTITIES for t, v in e[q].items()})
    for dn in DEFECTS:
        np.savez_compressed(out + f"_defect_{dn}.npz", **{k: np.asarray(v).astype(np.float32) for k, v in defects[dn].items()})
    for root, _, files in os.walk(d):
        for fn in files:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for fn in os.listdir(HERE):
        if fn.startswith(NAME + "_") and fn.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn
    print(NAME, "written:", json.dumps(summary))


if __name__ == "__main__":
    main()
