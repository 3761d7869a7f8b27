"""Writes the decoder-reranker fixtures under tests/golden/ (run on a machine with transformers; CPU):

  qwen3_rerank_d64_r1/, qwen3_rerank_d128_r2/   random ``Qwen3ForSequenceClassification`` checkpoint directories (one label; hidden
                                  256; head_dim 64 with GQA ratio 1, head_dim 128 with ratio 2): config.json, sharded
                                  model.safetensors (every file under 1 MiB), the word-level tokenizer.json of the embedder fixtures
                                  (pair template ``$A <|endoftext|> $B <|endoftext|>``).  The first names ``pad_token_id`` = the
                                  ``<|endoftext|>`` id the tokenizer appends, so every tokenised pair is pooled at the token BEFORE
                                  its last one (transformers pools the rightmost non-pad token); the second has ``pad_token_id: null``
                                  (the last token is pooled).
  qwen3_rerank_<dir>_expected.npz ragged token-id inputs (flat ``ids`` + ``lens``) and, per sequence, the pooled logit of
                                  ``logit_fp32``      the fp32 transformers model, one sequence per call (no padding enters),
                                  ``logit_bf16/fp16`` the same model with weights and activations cast to that type (each cast afresh
                                                      from the fp32 weights), run on the CPU,
                                  ``logit_last``      fp32, pooled at the TRUE last token (a defect reference where they differ),
                                  ``logit_nonorm``    fp32, the final norm left out (a defect reference),
                                  ``pool_pos``        the pooled position within each sequence;
                                  plus ``pair_query`` / ``pair_passage`` strings and ``pair_logit`` (fp32, tokenised by the fixture
                                  tokenizer) for the surface test.

    python tests/golden/make_qwen3_rerank_golden.py
"""
import copy
import json
import os

import numpy as np
import torch

from make_qwen3_golden import VOCAB, write_tokenizer

HERE = os.path.dirname(os.path.abspath(__file__))
EOS = VOCAB - 1
REQUIRED_LENGTHS = [1, 2, 15, 16, 17, 33, 129, 257, 600]
FIXTURES = {
    "qwen3_rerank_d64_r1": dict(num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, head_dim=64, seed=21,
                                pad_token_id=EOS),
    "qwen3_rerank_d128_r2": dict(num_hidden_layers=3, num_attention_heads=2, num_key_value_heads=1, head_dim=128, seed=22,
                                 pad_token_id=None),
}
PAIRS = [("w5 w17 w3", "w99 w5 w200 w17 w31 w8 w3"), ("w5 w17 w3", "w300 w301 w12"), ("w1", "w2"),
         ("w40 w41 w42 w43 w44 w45", "w7"), ("w250 w9", " ".join(f"w{(7 * i) % 382}" for i in range(90))),
         (" ".join(f"w{(11 * i) % 382}" for i in range(40)), " ".join(f"w{(13 * i + 5) % 382}" for i in range(150)))]


def sequences(rng):
    """>= 40 ragged sequences: the required lengths, random ones, some ENDING in one to three pad (<|endoftext|>) ids, one with a
    pad id in the middle, and two that hold nothing else."""
    body = lambda n: rng.integers(0, VOCAB - 2, n)          # noqa: E731
    seqs = [np.append(body(n - 1), EOS) if n > 2 else body(n) for n in REQUIRED_LENGTHS]
    seqs += [body(int(n)) for n in rng.integers(3, 120, 22)]
    seqs += [np.concatenate([body(int(n)), np.full(k, EOS)]) for n, k in ((4, 1), (15, 1), (14, 2), (30, 3), (64, 1), (97, 2))]
    inner = body(40)
    inner[17] = EOS
    seqs += [inner, np.full(1, EOS), np.full(5, EOS)]
    return [s.astype(np.int32) for s in seqs]


def pooled_position(ids, pad):
    """transformers' rule (GenericForSequenceClassification.forward), restated for the checks below."""
    if pad is None:
        return len(ids) - 1
    keep = np.nonzero(ids != pad)[0]
    return int(keep[-1]) if keep.size else 0


def main():
    from tokenizers import Tokenizer
    from transformers import Qwen3Config, Qwen3ForSequenceClassification

    for name, spec in FIXTURES.items():
        spec = dict(spec)
        seed, pad = spec.pop("seed"), spec["pad_token_id"]
        torch.manual_seed(seed)
        cfg = Qwen3Config(vocab_size=VOCAB, hidden_size=256, intermediate_size=128, max_position_embeddings=1024,
                          rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False, attention_bias=False, num_labels=1,
                          **spec)
        model = Qwen3ForSequenceClassification(cfg).eval().to(torch.float32)
        with torch.no_grad():
            for n, p in model.named_parameters():   # trained-model-like scales: norms around 1, not exactly 1
                if n.endswith("norm.weight"):
                    p.copy_(1 + 0.1 * torch.randn_like(p))
            # a head at the 0.02 init scale gives scores bunched at 0.5 that test nothing
            model.score.weight.copy_(0.15 * torch.randn_like(model.score.weight))
            if pad is not None:   # Embedding(padding_idx=) zeroed this row; trained checkpoints carry ordinary values there
                model.model.embed_tokens.weight[pad].copy_(0.02 * torch.randn(cfg.hidden_size))
        sd = model.state_dict()
        assert sorted(k for k in sd if not k.startswith("model.")) == ["score.weight"] and tuple(sd["score.weight"].shape) == (1, 256)
        d = os.path.join(HERE, name)
        os.makedirs(d, exist_ok=True)
        model.save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
        write_tokenizer(os.path.join(d, "tokenizer.json"))
        with open(os.path.join(d, "config.json")) as f:
            saved = json.load(f)
        assert saved["architectures"] == ["Qwen3ForSequenceClassification"] and saved["pad_token_id"] == pad

        rng = np.random.default_rng(seed)
        seqs = sequences(rng)
        lens = [len(s) for s in seqs]
        assert len(seqs) >= 40 and set(REQUIRED_LENGTHS) <= set(lens) and max(lens) > 512
        assert sum(1 for s in seqs if s[-1] == EOS and (s != EOS).any() and len(s) > 2) >= 4
        assert sum(1 for s in seqs if (s == EOS).all()) >= 1

        pre_norm = {}
        model.model.norm.register_forward_hook(lambda m, a, out: pre_norm.__setitem__("x", a[0]))
        w = model.score.weight[0]

        def logits_of(m, tokens):
            with torch.no_grad():
                return [float(m(input_ids=torch.from_numpy(s.astype(np.int64))[None]).logits[0, 0]) for s in tokens]

        fp32 = logits_of(model, seqs)
        pos = [pooled_position(s, pad) for s in seqs]
        last, nonorm = [], []
        with torch.no_grad():
            for s, p in zip(seqs, pos):
                h = model.model(input_ids=torch.from_numpy(s.astype(np.int64))[None]).last_hidden_state[0]
                assert abs(float(h[p] @ w) - fp32[len(last)]) <= 1e-5 * max(1.0, abs(fp32[len(last)])), "pooled-token rule"
                last.append(float(h[-1] @ w))
                nonorm.append(float(pre_norm["x"][0, p] @ w))
        low = {}
        for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            low[key] = logits_of(copy.deepcopy(model).to(dt), seqs)      # cast afresh from the fp32 weights
        score = 1 / (1 + np.exp(-np.asarray(fp32)))
        assert score.min() < 0.1 and score.max() > 0.9, (score.min(), score.max())

        tk = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
        pair_ids = [np.asarray(tk.encode(q, p).ids, dtype=np.int32) for q, p in PAIRS]
        assert all(i[-1] == EOS for i in pair_ids)
        np.savez_compressed(
            os.path.join(HERE, f"{name}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(lens, dtype=np.int32),
            logit_fp32=np.asarray(fp32, dtype=np.float64), logit_bf16=np.asarray(low["bf16"], dtype=np.float64),
            logit_fp16=np.asarray(low["fp16"], dtype=np.float64), logit_last=np.asarray(last, dtype=np.float64),
            logit_nonorm=np.asarray(nonorm, dtype=np.float64), pool_pos=np.asarray(pos, dtype=np.int32),
            pair_query=np.asarray([q for q, _ in PAIRS]), pair_passage=np.asarray([p for _, p in PAIRS]),
            pair_logit=np.asarray(logits_of(model, pair_ids), dtype=np.float64))
        for root, _, files in os.walk(d):
            for fn in files:
                assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
        e = {k: float(np.abs(np.asarray(v) - np.asarray(fp32)).max()) for k, v in low.items()}
        print(name, "written:", len(seqs), "sequences, fp32 logits", min(fp32), "..", max(fp32), "e_ref", e)


if __name__ == "__main__":
    main()
