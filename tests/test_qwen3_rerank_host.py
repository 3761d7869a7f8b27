"""CPU: the decoder reranker's host side -- ``Qwen3ForSequenceClassification`` config and checkpoint-name mapping, which token is
pooled (``encoder.pooled_rows`` against the rows the fixtures record from transformers), and the surface's token-source and
template rules.  Fixtures: tests/golden/make_qwen3_rerank_golden.py.  No GPU needed."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"qwen3_rerank_d64_r1": 383, "qwen3_rerank_d128_r2": None}     # directory -> pad_token_id


def _config(name):
    with open(os.path.join(GOLDEN, name, "config.json")) as f:
        return json.load(f)


def _sequences(name):
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return [z["ids"][f:f + n] for f, n in zip(first, lens)], z


@pytest.mark.parametrize("name", FIXTURES)
def test_classification_config_names_one_label_and_the_pad_token(name):
    from tensor_truth_amd import weights

    d = _config(name)
    assert d["architectures"] == ["Qwen3ForSequenceClassification"]
    cfg = weights._config_from_hf(d)
    assert cfg.arch == "qwen3" and cfg.num_labels == 1 and cfg.pad_token_id == FIXTURES[name]
    assert cfg.pad_id == 0                                   # the filler of rows of no sequence: not the checkpoint's pad token
    # the same sizes under an embedder's architecture: no head, whatever the caller would like (want_head only sets a default
    # for the encoder family)
    emb = weights._config_from_hf(dict(d, architectures=["Qwen3Model"]), 1)
    assert emb.num_labels == 0 and emb.pad_token_id == FIXTURES[name]


def test_embedder_config_is_untouched_by_the_new_field():
    from tensor_truth_amd import weights
    from tensor_truth_amd.decoder import QWEN3_EMBEDDING_0_6B, DecoderConfig

    d = {"architectures": ["Qwen3ForCausalLM"], "model_type": "qwen3", "vocab_size": 151669, "hidden_size": 1024,
         "num_hidden_layers": 28, "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128,
         "intermediate_size": 3072, "max_position_embeddings": 32768, "rms_norm_eps": 1e-6, "rope_theta": 1000000}
    assert "pad_token_id" not in d and weights._config_from_hf(d) == QWEN3_EMBEDDING_0_6B
    assert DecoderConfig().pad_token_id is None and QWEN3_EMBEDDING_0_6B.num_labels == 0


@pytest.mark.parametrize("change", [dict(num_labels=3), dict(id2label={"0": "a", "1": "b"})], ids=lambda c: next(iter(c)))
def test_more_than_one_label_is_refused(change):
    from tensor_truth_amd import weights

    with pytest.raises(ValueError, match="single-label"):
        weights._config_from_hf(dict(_config("qwen3_rerank_d64_r1"), **change))


@pytest.mark.parametrize("name", FIXTURES)
def test_state_names_of_a_classification_checkpoint(name):
    from tensor_truth_amd import weights
    from tensor_truth_amd.decoder import state_names
    from tensor_truth_amd.encoder import _strip_prefix

    cfg = weights._config_from_hf(_config(name))
    sd = _strip_prefix(weights.load_state(os.path.join(GOLDEN, name)))
    assert set(sd) == set(state_names(cfg)) and "score.weight" in sd
    assert tuple(sd["score.weight"].shape) == (1, cfg.hidden)
    import dataclasses

    assert "score.weight" not in state_names(dataclasses.replace(cfg, num_labels=0))


def test_score_bias_and_other_extras_are_refused():
    """transformers' head is Linear(H, 1, bias=False): a score.bias means another head, refused like any tensor the forward would
    not read (the check runs before anything touches a device)."""
    import torch

    from tensor_truth_amd import weights
    from tensor_truth_amd.decoder import DecoderWeights

    name = "qwen3_rerank_d64_r1"
    cfg = weights._config_from_hf(_config(name))
    sd = weights.load_state(os.path.join(GOLDEN, name))
    with pytest.raises(NotImplementedError, match="score.bias"):
        DecoderWeights(cfg, dict(sd, **{"score.bias": torch.zeros(1)}), torch.device("cuda", 0))
    missing = {k: v for k, v in sd.items() if k != "score.weight"}
    with pytest.raises(ValueError, match="score.weight"):
        DecoderWeights(cfg, missing, torch.device("cuda", 0))


@pytest.mark.parametrize("name", FIXTURES)
def test_pooled_rows_are_transformers_rows(name):
    """The fixture records, per sequence, the position whose hidden state reproduces transformers' pooled logit (checked when it
    was written): ``pooled_rows`` names that position in a packed batch, in any order of the sequences."""
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import pack_tokens, pooled_rows

    cfg = weights._config_from_hf(_config(name))
    seqs, z = _sequences(name)
    want = z["pool_pos"].astype(np.int64)
    order = np.random.default_rng(5).permutation(len(seqs))
    for idx in (np.arange(len(seqs)), order):
        batch = pack_tokens([seqs[i] for i in idx], cfg)
        rows = pooled_rows(batch, cfg.pad_token_id)
        assert rows.dtype == np.int32 and (rows - batch.seq_start == want[idx]).all()
        assert (pooled_rows(batch, None) == batch.seq_start + batch.seq_len - 1).all()
    pad = FIXTURES[name]
    if pad is not None:
        ends_in_pad = [i for i, s in enumerate(seqs) if s[-1] == pad and (s != pad).any()]
        all_pad = [i for i, s in enumerate(seqs) if (s == pad).all()]
        assert len(ends_in_pad) >= 4 and all_pad
        assert all(want[i] < len(seqs[i]) - 1 and seqs[i][want[i]] != pad and (seqs[i][want[i] + 1:] == pad).all()
                   for i in ends_in_pad)
        assert all(want[i] == 0 for i in all_pad)
        inner = [i for i, s in enumerate(seqs) if s[-1] != pad and (s == pad).any()]
        assert inner and all(want[i] == len(seqs[i]) - 1 for i in inner)      # a pad id in the middle changes nothing
    else:
        assert (want == z["lens"] - 1).all()


def test_pooled_rows_follow_truncation():
    from tensor_truth_amd.decoder import DecoderConfig
    from tensor_truth_amd.encoder import pack_tokens, pooled_rows

    cfg = DecoderConfig(vocab_size=100, hidden=256, layers=1, heads=4, ffn=128, max_pos=64, kv_heads=4, head_dim=64, pad_token_id=9)
    batch = pack_tokens([[1, 2, 3, 4, 9, 9, 5, 9], [9, 9], [7]], cfg, max_len=6)
    assert (batch.seq_len == [6, 2, 1]).all()
    assert (pooled_rows(batch, 9) - batch.seq_start == [3, 0, 0]).all()       # [1 2 3 4 9 9] -> the 4; all pad -> 0


def _surface(arch="qwen3", **templates):
    """A reranker surface without a device: only what the token-source and template rules read."""
    from tensor_truth_amd.decoder import DecoderConfig
    from tensor_truth_amd.encoder import BGE_RERANKER_V2_M3
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank as R
    from tensor_truth_amd.tokenization import HashTokenizer

    r = R.__new__(R)
    r.config = DecoderConfig(num_labels=1) if arch == "qwen3" else BGE_RERANKER_V2_M3
    r._use_types = False
    r._tokenizer = HashTokenizer("xlmr", 1000)
    r._token_source = None
    r.query_template = R._template(templates, "query_template", "query")
    r.document_template = R._template(templates, "document_template", "document")
    return r


def test_a_decoder_reranker_takes_no_stored_passage_ids():
    from tensor_truth_amd.tokenization import tokenizer_signature

    enc = _surface("xlmr")
    sig = tokenizer_signature(enc._tokenizer)
    assert enc.accepts_token_source(sig)                       # the encoder family is unchanged
    dec = _surface("qwen3")
    assert not dec.accepts_token_source(sig) and not dec.attach_token_source(lambda i: None, sig)
    assert dec._token_source is None
    assert not _surface("xlmr", document_template="D: {document}").accepts_token_source(sig)


def test_templates_format_both_sides():
    r = _surface(query_template="<Instruct>: judge\n<Query>: {query}", document_template="<Document>: {document} </s>")
    assert r.format_pair("a b", "c") == ("<Instruct>: judge\n<Query>: a b", "<Document>: c </s>")
    assert r._formatted([("q", "d")]) == [("<Instruct>: judge\n<Query>: q", "<Document>: d </s>")]
    plain = _surface()
    pairs = [("q", "d")]
    assert plain.format_pair("q", "d") == ("q", "d") and plain._formatted(pairs) is pairs     # default: the reference's strings
    only_q = _surface(query_template="Q: {query}")
    assert only_q.format_pair("x", "y") == ("Q: x", "y")
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank as R

    for bad in ({"query_template": "no field"}, {"query_template": "{document}"}, {"document_template": "{document} {other}"},
                {"document_template": 5}):
        with pytest.raises(ValueError, match="template"):
            key = next(iter(bad))
            R._template(bad, key, key.split("_")[0])
