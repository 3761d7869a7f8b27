"""Writes the BGE-M3 lexical-head fixtures under tests/golden/ (run on a machine with transformers; CPU, nothing downloaded).

[UPSTREAM-K] The checkpoint file ``sparse_linear.pt`` (a torch-pickled state dict, ``weight`` [1][H] and ``bias`` [1]) and the
semantics -- token weight relu(<w, h_i> + b) over the last hidden state, the maximum per token id, the ids of <s> </s> <pad> <unk> and
weights <= 0 left out, lex(q, d) = sum over shared ids of q_w * d_w, hybrid = (w_dense * dense + w_lex * lex) / (w_dense + w_lex) --
are written here from knowledge of FlagEmbedding's ``BGEM3FlagModel``, which is not installed.  The ENCODER arithmetic is pinned to a
class that is, and a failed pin stops the script: ``XLMRobertaModel`` (eager attention) equals the fp64 forward restated below
(positions pad_id + 1 + i, one token type) on every text.

  m3_l2/                    config.json (model_type xlm-roberta: 2 layers, hidden 128, 2 heads of 64, ffn 256, 66 positions, vocabulary
                            600, pad id 1), model.safetensors (XLMRobertaModel's names, pooler included), sparse_linear.pt, and a
                            word-level tokenizer.json (<s> <pad> </s> <unk> at 0 .. 3, then w0 .. w595).  The weights are rounded
                            to fp16 before anything is computed, with scales chosen so that the model is LEXICAL, as a trained
                            one is: keys equal queries and are sharpened, so a token attends to itself and its repetitions and
                            its row stays a function of the token (small position table), while <s>'s query is projected out in
                            the first layer, so the CLS row attends evenly and becomes the text's content -- dense scores then
                            follow word overlap.  The head is tilted so that <s>, </s> and <unk> weigh clearly more than 0 (a
                            defect that keeps them shows), with a bias negative enough that a visible share of tokens weighs 0.
  m3_l2_expected.npz        the token ids (with <s> and </s>) and the texts of 4 queries (6, 7, 9 and 8 words; no two share a word;
                            queries 0 and 2 end with a stopword whose weight is 0, query 0 holds an out-of-vocabulary word) and
                            24 passages: passage i belongs to query i // 6 and holds the first 6/6 .. 1/6 of its words, two of them
                            twice, then filler words no query holds, drawn from a small pool so that they repeat; bodies of 1 to
                            67 words (one passage is longer than the 64-token limit and truncated, one fills it exactly); three
                            passages hold the out-of-vocabulary word.  A passage's lexical score is therefore > 0 for its own
                            query and exactly 0 for the other three.  Words are substituted until every query word weighs at
                            least QUERY_PRE in every text, every stopword lies below STOP_PRE and no word's pre-activation is
                            within MARGIN of zero.  In fp64 arithmetic: ``weights`` [28][600] (a text's lexical weight per token
                            id, 0 = not held), ``preact_margin`` (the smallest |pre-activation| of any token but <s>, </s>: the
                            kept set of an implementation within it of fp64 is the fp64 set), ``dense`` [28][128], ``lex`` /
                            ``dense_score`` / ``hybrid`` [4][24] with ``hybrid_weights`` (0.4, 0.2: upstream's example);
                            ``e_<quantity>_<type>`` for the quantities weights, dense, lex, dense_score, hybrid and the types
                            bf16, fp16: the largest deviation from fp64 of the same torch modules (XLMRobertaModel, Linear + relu,
                            normalize) run in that type on the CPU, with the scores evaluated in fp64 ON those vectors (the error
                            the type puts into the vectors alone) -- the dense vectors rounded to bf16 first, which is how the
                            store keeps them for every type.
  m3_l2_defect_<d>.npz      ``weights``, ``lex`` and ``hybrid`` in fp64 arithmetic (stored as fp32) under the defects an implementation
                            could have --
                              ``keepspecials``  <s> and </s> kept in the lexical vectors,
                              ``sum``           an id's occurrences summed instead of maximised,
                              ``norelu``        negative weights kept,
                              ``nobias``        the bias not added,
                              ``keepunk``       <unk> kept.

The GPU test bounds |hip - fp64| by 2 e_<type> (DESIGN.md 4.8's factor for a second 16-bit implementation) and wants every defect
quantity outside that bound, which holds iff the defect is more than 4 e from fp64 -- asserted below for every quantity and both
types.  Also asserted: ``preact_margin`` > 2 e_weights of the coarser type (no id is left out of the set comparison); for every
query, consecutive fp64 scores among its top 6 differ by more than 4 e of the coarser type -- for the hybrid score over all passages,
for the lexical score over the passages that score > 0 -- so the tests can demand the fp64 order; and every query's best passage by
the dense score stands more than 4 e clear of the second (dense scores of a two-layer model lie close together: the test demands
the fp64 dense order of exactly those pairs of passages whose fp64 scores differ by more than 4 e).

    python tests/golden/make_m3_golden.py
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
NAME = "m3_l2"
SPECIALS = ["<s>", "<pad>", "</s>", "<unk>"]
BOS, PAD, EOS, UNK = range(4)
FIRST_WORD = len(SPECIALS)
VOCAB = 600
HIDDEN, HEADS, FFN, LAYERS, MAX_POS, EPS = 128, 2, 256, 2, 66, 1e-5
MAX_LEN = MAX_POS - (PAD + 1)          # 64 tokens with <s> and </s>
QUERY_BODIES = [6, 7, 9, 8]             # words per query; queries 0 and 2 end with one more word, a stopword (weight 0)
STOP_QUERIES = (0, 2)
# passage i belongs to query i // 6 and holds the first TAKE(i % 6) of its words, then DOC_EXTRA[i] filler words no query holds
DOC_EXTRA = [3, 9, 16, 24, 33, 0, 4, 14, 23, 41, 59, 1, 2, 8, 26, 45, 64, 0, 0, 5, 12, 22, 30, 56]
OOV_QUERY, OOV_DOCS = 0, (0, 1, 2)
SEED = 97
QK_SHARPEN, VO_GAIN, BIAS_STD, LN_BIAS_STD, MLP_GAIN, POS_GAIN = 5.0, 5.0, 0.1, 0.03, (1.0, 0.5), 0.15
HEAD_STD, HEAD_BIAS = 0.16, -1.8
SPECIAL_PRE = {BOS: 2.0, EOS: 1.5, UNK: 1.8}   # the head is tilted so that these tokens' pre-activations sit near these values: a
#                                                # defect that keeps them then shows (a random head leaves some of them below 0)
BOS_GAIN = 0.2                         # <s>'s own embedding against the words': the CLS row is what it attends to
STOP_PRE = -1.2                        # every occurrence of a stopword lies below this
QUERY_PRE = 2.0                        # every occurrence of a query's word weighs at least this much: one shared word is a visible step
MARGIN = 0.15                          # no non-special token's pre-activation is closer to 0 (words are substituted until so)
HYBRID = (0.4, 0.2)
FACTOR = 2.0
DEFECTS = ["keepspecials", "sum", "norelu", "nobias", "keepunk"]
QUANTITIES = ["weights", "dense", "lex", "dense_score", "hybrid"]


def layout(body):
    """<s> body </s>, cut to the model's limit keeping the closing token (what the embedder's tokenizer call does)."""
    ids = [BOS] + [int(t) for t in body] + [EOS]
    return ids if len(ids) <= MAX_LEN else ids[: MAX_LEN - 1] + [EOS]


def take_count(n_words, k):
    return max(1, (n_words * (6 - k) + 5) // 6)


def bodies(rng):
    """-> (query bodies, passage bodies, stopwords).  No two queries share a word and no filler word is a query's, so a passage's
    lexical score is graded by construction for its own query and exactly 0 for the others."""
    perm = rng.permutation(np.arange(FIRST_WORD, VOCAB)).astype(np.int32)
    n_qw = sum(QUERY_BODIES) + len(STOP_QUERIES)
    qwords, filler = perm[:n_qw], perm[n_qw:n_qw + 200]
    qs, stops, at = [], {}, 0
    for qi, n in enumerate(QUERY_BODIES):
        qs.append(qwords[at:at + n].copy())
        at += n
        if qi in STOP_QUERIES:
            stops[qi] = int(qwords[at])
            at += 1
    ds = []
    for i, extra in enumerate(DOC_EXTRA):
        qi, k = i // 6, i % 6
        take = qs[qi][: take_count(len(qs[qi]), k)]
        # the filler comes from a small pool, so words repeat inside a text; the query's first two words stand twice
        pool = rng.choice(filler, max(2, extra // 3))
        tail = rng.choice(pool, extra).astype(np.int32)
        tail[: min(2, extra, len(take))] = take[: min(2, extra, len(take))]
        if qi in stops and extra >= 4:
            tail[3] = stops[qi]
        ds.append(np.concatenate([take, tail]).astype(np.int32))
    for qi, w in stops.items():
        qs[qi] = np.append(qs[qi], np.int32(w))
    qs[OOV_QUERY] = np.insert(qs[OOV_QUERY], 1, UNK).astype(np.int32)
    for i in OOV_DOCS:
        ds[i] = np.append(ds[i], [UNK, ds[i][-1], UNK]).astype(np.int32)
    return qs, ds, set(stops.values())


def write_tokenizer(path):
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {t: i for i, t in enumerate(SPECIALS)}
    vocab.update({f"w{i}": FIRST_WORD + i for i in range(VOCAB - FIRST_WORD)})
    assert len(vocab) == VOCAB
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.add_special_tokens(SPECIALS)
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>",
                                                      special_tokens=[("<s>", BOS), ("</s>", EOS)])
    tk.save(path)


def text_of(body):
    return " ".join("oov" if t == UNK else f"w{int(t) - FIRST_WORD}" for t in body)


# ---- the model, restated in fp64 ---------------------------------------------------------------------------------------------------
def layer_norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def forward64(sd, ids):
    n = len(ids)
    lin = lambda x, name: x @ sd[name + ".weight"].T + sd[name + ".bias"]  # noqa: E731
    ln = lambda x, name: layer_norm(x, sd[name + ".weight"], sd[name + ".bias"])  # noqa: E731
    x = (sd["embeddings.word_embeddings.weight"][torch.as_tensor(np.asarray(ids, dtype=np.int64))]
         + sd["embeddings.position_embeddings.weight"][PAD + 1:PAD + 1 + n] + sd["embeddings.token_type_embeddings.weight"][0])
    x = ln(x, "embeddings.LayerNorm")
    dh = HIDDEN // HEADS
    for i in range(LAYERS):
        p = f"encoder.layer.{i}."
        q, k, v = (lin(x, p + f"attention.self.{m}").view(n, HEADS, dh) for m in ("query", "key", "value"))
        s = torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(dh)
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, HIDDEN)
        x = ln(x + lin(a, p + "attention.output.dense"), p + "attention.output.LayerNorm")
        f = lin(torch.nn.functional.gelu(lin(x, p + "intermediate.dense")), p + "output.dense")
        x = ln(x + f, p + "output.LayerNorm")
    return x


def token_weights(ids, pre, defect=None):
    """Per-token pre-activations (bias added) of one text -> its lexical weights as a dense [VOCAB] vector (0 = not held)."""
    out = np.zeros(VOCAB)
    seen = set()
    left_out = {BOS, EOS, PAD, UNK}
    if defect == "keepspecials":
        left_out -= {BOS, EOS}
    if defect == "keepunk":
        left_out -= {UNK}
    for t, v in zip(ids, pre):
        if t in left_out:
            continue
        if defect != "norelu":
            v = max(v, 0.0)
        if defect == "sum":
            out[t] += v
        elif t not in seen or v > out[t]:
            out[t] = v
        seen.add(t)
    if defect != "norelu":
        out[out < 0] = 0.0
    return out


def scores_of(weights, dense, n_q):
    """-> (lex, dense_score, hybrid) [n_q][n_d] from the texts' weight vectors and L2-normalised dense vectors (queries first)."""
    lex = weights[:n_q] @ weights[n_q:].T
    ds = dense[:n_q] @ dense[n_q:].T
    return lex, ds, (HYBRID[0] * ds + HYBRID[1] * lex) / (HYBRID[0] + HYBRID[1])


def reference(hiddens, seqs, w, b, n_q, defect=None):
    bias = 0.0 if defect == "nobias" else b
    weights = np.stack([token_weights(ids, (h @ w + bias).numpy(), defect) for ids, h in zip(seqs, hiddens)])
    dense = np.stack([(h[0] / h[0].norm().clamp_min(1e-12)).numpy() for h in hiddens])
    return (weights, dense) + scores_of(weights, dense, n_q)


def model_hidden(model, ids):
    with torch.no_grad():
        return model(input_ids=torch.as_tensor(np.asarray(ids, dtype=np.int64))[None]).last_hidden_state[0]


def top_gap(rows, positive_only=False):
    gaps = []
    for row in rows:
        r = np.sort(row[row > 0] if positive_only else row)[::-1][:6]
        if len(r) > 1:
            gaps.append(float(np.min(-np.diff(r))))
    return min(gaps)


def main():
    from safetensors.torch import save_file
    from transformers import XLMRobertaConfig, XLMRobertaModel

    from tensor_truth_amd import lexical as tl

    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    qs, ds, stops = bodies(rng)
    n_q = len(qs)
    cfg = XLMRobertaConfig(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=FFN,
                           num_hidden_layers=LAYERS, type_vocab_size=1, max_position_embeddings=MAX_POS, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, layer_norm_eps=EPS, hidden_act="gelu", pad_token_id=PAD, bos_token_id=BOS,
                           eos_token_id=EOS)
    cfg._attn_implementation = "eager"
    model = XLMRobertaModel(cfg, add_pooling_layer=True).eval().to(torch.float32)
    assert cfg._attn_implementation == "eager"
    head = torch.nn.Linear(HIDDEN, 1)
    with torch.no_grad():
        for n, p in model.named_parameters():        # trained-model-like scales: nothing exactly 1 or exactly 0
            if "LayerNorm.weight" in n:
                p.copy_(1 + 0.1 * torch.randn_like(p))
            elif "LayerNorm.bias" in n:
                p.copy_(LN_BIAS_STD * torch.randn_like(p))
            elif n.endswith(".bias"):
                p.copy_(BIAS_STD * torch.randn_like(p))
        emb = model.embeddings
        emb.word_embeddings.weight[PAD].copy_(0.02 * torch.randn(HIDDEN))       # Embedding(padding_idx=) zeroed this row
        emb.position_embeddings.weight.mul_(POS_GAIN)
        emb.word_embeddings.weight[BOS].mul_(BOS_GAIN)
        # keys = queries, sharpened: a token attends to itself (and to its repetitions), so its row stays a function of the token --
        # except <s> in the first layer, whose query is projected out (it attends evenly: the CLS row becomes the text's content)
        cls0 = torch.nn.functional.layer_norm(emb.word_embeddings.weight[BOS] + emb.position_embeddings.weight[PAD + 1]
                                              + emb.token_type_embeddings.weight[0], (HIDDEN,), emb.LayerNorm.weight,
                                              emb.LayerNorm.bias, EPS)
        for li, layer in enumerate(model.encoder.layer):
            att = layer.attention
            att.self.query.weight.mul_(QK_SHARPEN)
            att.self.query.bias.zero_()
            if li == 0:
                att.self.query.weight.sub_(torch.outer(att.self.query.weight @ cls0, cls0) / (cls0 @ cls0))
            att.self.key.weight.copy_(att.self.query.weight)
            att.self.key.bias.zero_()
            for m in (att.self.value, att.output.dense):
                m.weight.mul_(VO_GAIN)
            layer.intermediate.dense.weight.mul_(MLP_GAIN[0])
            layer.output.dense.weight.mul_(MLP_GAIN[1])
        head.weight.normal_(0.0, HEAD_STD)
        head.bias.fill_(HEAD_BIAS)
        model = model.half().float()                 # the stored weights ARE the model's: fp16 values
        probe = [layout(b) for b in qs + ds]
        hid = [model_hidden(model, ids) for ids in probe]
        mean = torch.cat(hid).mean(0)
        for tok, want in SPECIAL_PRE.items():
            rows = torch.stack([h[i] for ids, h in zip(probe, hid) for i, t in enumerate(ids) if t == tok])
            u = rows.mean(0) - mean
            now = float((rows @ head.weight[0] + head.bias[0]).mean())
            head.weight[0].add_((want - now) * u / (u @ rows.mean(0)))
        head = head.half().float()
    stored = {k: v.half().contiguous() for k, v in model.state_dict().items() if k != "embeddings.position_ids"}
    sd64 = {k: v.double() for k, v in stored.items()}
    w64, b64 = head.weight.detach().double()[0], float(head.bias.detach().double()[0])

    # words whose pre-activation comes within MARGIN of zero anywhere are substituted in every text (the overlap structure stays)
    # a replacement is drawn among the words whose pre-activation standing alone is well on the wanted side
    alone = {t: float(forward64(sd64, [BOS, t, EOS])[1] @ w64 + b64) for t in range(FIRST_WORD, VOCAB)}
    spare = rng.permutation(np.arange(FIRST_WORD, VOCAB)).tolist()
    if os.environ.get("M3_GOLDEN_VERBOSE"):
        print("pre-activation of a word standing alone: quantiles", np.quantile(list(alone.values()), [0, 0.05, 0.25, 0.5, 0.75, 0.95, 1]))
    for _ in range(200):
        seqs = [layout(b) for b in qs + ds]
        hiddens = [forward64(sd64, ids) for ids in seqs]
        qwords = {int(t) for b in qs for t in b} - stops
        bad = {int(t) for ids, h in zip(seqs, hiddens) for t, v in zip(ids, (h @ w64 + b64).tolist())
               if t >= FIRST_WORD and (abs(v) < MARGIN or (t in qwords and v < QUERY_PRE) or (t in stops and v > STOP_PRE))}
        if os.environ.get("M3_GOLDEN_VERBOSE"):
            print("round", _, "words to substitute:", len(bad), "query", len(bad & qwords), "stop", len(bad & stops))
        if not bad:
            break
        used = {int(t) for b in qs + ds for t in b}
        for t in sorted(bad):
            fits = ((lambda v: v < STOP_PRE - 0.5) if t in stops else (lambda v: v > QUERY_PRE + 0.5) if t in qwords
                    else (lambda v: abs(v) > MARGIN + 0.3))
            new = next(x for x in spare if x not in used and fits(alone[x]))
            used.add(new)
            for b in qs + ds:
                b[b == t] = new
            if t in stops:
                stops = (stops - {t}) | {new}
    else:
        raise AssertionError("the substitution did not converge")
    seqs = [layout(b) for b in qs + ds]
    assert max(len(s) for s in seqs) == MAX_LEN and sum(len(b) + 2 > MAX_LEN for b in ds) == 1
    assert any(len(set(s)) < len(s) for s in seqs[n_q:]), "no text repeats a token"
    hiddens = [forward64(sd64, ids) for ids in seqs]
    pre_all = [(h @ w64 + b64).numpy() for h in hiddens]
    margin = min(float(abs(v)) for ids, pre in zip(seqs, pre_all) for t, v in zip(ids, pre) if t not in (BOS, EOS, PAD))
    zero_share = float(np.mean([v <= 0 for ids, pre in zip(seqs, pre_all) for t, v in zip(ids, pre) if t >= FIRST_WORD]))
    # (<unk> cannot be substituted: its margin is checked against 2 e below, with everything else)
    assert 0.1 < zero_share < 0.7, zero_share

    # pin: XLMRobertaModel == the forward restated above; the package's helpers == what is restated here
    m64 = copy.deepcopy(model).double()
    pin = max(float((model_hidden(m64, ids) - h).abs().max()) for ids, h in zip(seqs, hiddens))
    assert pin < 1e-10, pin

    weights, dense, lex, dscore, hybrid = reference(hiddens, seqs, w64, b64, n_q)
    own = np.arange(len(ds))[None, :] // 6 == np.arange(n_q)[:, None]
    assert (lex[~own] == 0).all() and (lex[own] > 0).all(), "a query must share weighted ids with its own six passages only"
    assert weights[OOV_QUERY, UNK] == 0 and all((weights[n_q + i] > 0).sum() < len(set(seqs[n_q + i])) for i in OOV_DOCS)

    e = {q: {} for q in QUANTITIES}
    for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m16, h16 = copy.deepcopy(model).to(dt), copy.deepcopy(head).to(dt)        # cast afresh from the stored weights
        hid = [model_hidden(m16, ids) for ids in seqs]
        with torch.no_grad():
            pre = [h16(h)[:, 0].double().numpy() for h in hid]
            d16 = np.stack([torch.nn.functional.normalize(h[0].float(), p=2, dim=-1, eps=1e-12).to(dt).double().numpy() for h in hid])
        w16 = np.stack([token_weights(ids, p) for ids, p in zip(seqs, pre)])
        # (the store keeps a passage's dense row in bf16 whatever the encoder's type, and the query's is rounded to match)
        stored16 = torch.from_numpy(d16).to(torch.bfloat16).double().numpy()
        got = (w16, d16) + scores_of(w16, stored16, n_q)
        for q, a, r in zip(QUANTITIES, got, (weights, dense, lex, dscore, hybrid)):
            e[q][key] = float(np.abs(a - r).max())
    coarse = {q: max(e[q].values()) for q in QUANTITIES}
    assert all(1e-6 < v < 2.0 for q in QUANTITIES for v in e[q].values()), e
    failed = []
    if not margin > FACTOR * coarse["weights"]:
        failed.append(f"pre-activation margin {margin:.4f} inside 2 e_weights = {FACTOR * coarse['weights']:.4f}")

    # (dense scores of a two-layer model lie close together: only every query's best passage is asked to stand clear; the test
    # demands the fp64 order of exactly those pairs whose fp64 dense scores differ by more than 4 e)
    gaps = {"hybrid": top_gap(hybrid), "dense_score": min(float(r[0] - r[1]) for r in np.sort(dscore, 1)[:, ::-1]),
            "lex": top_gap(lex, positive_only=True)}
    for q, g in gaps.items():
        if not g > 2 * FACTOR * coarse[q]:
            failed.append(f"top-6 {q} scores only {g:.5f} apart: 4 e = {2 * FACTOR * coarse[q]:.5f}")

    defects, dgaps = {}, {}
    for dn in DEFECTS:
        dw, _, dl, _, dh = reference(hiddens, seqs, w64, b64, n_q, defect=dn)
        defects[dn] = {"weights": dw, "lex": dl, "hybrid": dh}
        for q, a, r in (("weights", dw, weights), ("lex", dl, lex), ("hybrid", dh, hybrid)):
            dgaps[f"{dn}:{q}"] = g = float(np.abs(a - r).max())
            if not g > 2 * FACTOR * coarse[q]:
                failed.append(f"defect {dn}:{q} is only {g:.5f} from fp64: inside 4 e = {2 * FACTOR * coarse[q]:.5f}")
    if failed:
        np.set_printoptions(precision=3, suppress=True, linewidth=200)
        print("dense_score top 7 per query:\n", np.sort(dscore, 1)[:, ::-1][:, :7], "\nlex top 7:\n", np.sort(lex, 1)[:, ::-1][:, :7],
              "\nhybrid top 7:\n", np.sort(hybrid, 1)[:, ::-1][:, :7])
    assert not failed, (failed, e, margin, zero_share, gaps, dgaps)

    # ---- write ------------------------------------------------------------------------------------------------------------------
    d = os.path.join(HERE, NAME)
    os.makedirs(d, exist_ok=True)
    save_file(stored, os.path.join(d, "model.safetensors"), metadata={"format": "pt"})
    torch.save({"weight": head.weight.detach().clone(), "bias": head.bias.detach().clone()}, os.path.join(d, tl.SPARSE_FILE))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"architectures": ["XLMRobertaModel"], "model_type": "xlm-roberta", "hidden_size": HIDDEN, "num_hidden_layers": LAYERS,
                   "num_attention_heads": HEADS, "intermediate_size": FFN, "vocab_size": VOCAB, "type_vocab_size": 1,
                   "layer_norm_eps": EPS, "max_position_embeddings": MAX_POS, "pad_token_id": PAD, "bos_token_id": BOS,
                   "eos_token_id": EOS, "hidden_act": "gelu", "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0,
                   "initializer_range": 0.02, "position_embedding_type": "absolute", "torch_dtype": "float16"}, f, indent=2)
    write_tokenizer(os.path.join(d, "tokenizer.json"))

    # the package's helpers read back what is restated here
    from tensor_truth_amd.tokenization import load_tokenizer

    tk = load_tokenizer(d, "xlmr", VOCAB)
    assert tl.special_ids(tk) == (BOS, EOS, PAD, UNK)
    assert tl.has_lexical_head(d)
    lw, lb = tl.load_sparse_head(d, HIDDEN)
    assert torch.equal(lw.double(), w64) and lb == b64
    texts = [text_of(b) for b in qs + ds]
    assert [tk.encode(t, MAX_LEN) for t in texts] == seqs, "the tokenizer's ids are not the layout restated here"

    out = os.path.join(HERE, NAME)
    np.savez_compressed(out + "_expected.npz", ids=np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]),
                        lens=np.asarray([len(s) for s in seqs], dtype=np.int32), n_queries=np.int32(n_q), texts=np.asarray(texts),
                        weights=weights, dense=dense, lex=lex, dense_score=dscore, hybrid=hybrid, hybrid_weights=np.asarray(HYBRID),
                        preact_margin=np.float64(margin), defects=np.asarray(DEFECTS),
                        **{f"e_{q}_{t}": np.float64(v) for q in QUANTITIES for t, v in e[q].items()})
    for dn in DEFECTS:
        np.savez_compressed(out + f"_defect_{dn}.npz", **{k: np.asarray(v).astype(np.float32) for k, v in defects[dn].items()})
    for root, _, files in os.walk(d):
        for fn in files:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for fn in os.listdir(HERE):
        if fn.startswith(NAME + "_") and fn.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn
    print(NAME, "written: pin XLMRobertaModel", pin, "; e", e, "; pre-activation margin", margin, "; zero share", zero_share,
          "; top-6 gaps", gaps, "; defect gaps", dgaps, "; lex range", float(lex.min()), float(lex.max()),
          "; hybrid range", float(hybrid.min()), float(hybrid.max()))


if __name__ == "__main__":
    main()
