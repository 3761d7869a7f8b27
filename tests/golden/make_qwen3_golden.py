"""Writes the decoder-embedder fixtures under tests/golden/ (run on a machine with transformers; CPU, fp32):

  qwen3_d64_r1/, qwen3_d128_r2/   random ``Qwen3Model`` checkpoint directories (hidden 256; head_dim 64 with GQA ratio 1, head_dim
                                  128 with ratio 2): config.json, sharded model.safetensors (every file under 1 MiB), a word-level
                                  tokenizer.json whose post-processor appends <|endoftext|>, 1_Pooling/config.json (last token) and
                                  config_sentence_transformers.json (query / document prompts);
  qwen3_<dir>_expected.npz        ragged token-id inputs (up to 600 tokens; flat ids + lengths) and the fp32 transformers
                                  model's last-token embeddings of them, L2-normalised.

    python tests/golden/make_qwen3_golden.py
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB = 384
LENGTHS = [1, 2, 15, 17, 31, 33, 64, 129, 257, 600]
QUERY_PROMPT = "Instruct: Given a question, retrieve passages that answer it\nQuery:"
FIXTURES = {
    "qwen3_d64_r1": dict(num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, head_dim=64, seed=11),
    "qwen3_d128_r2": dict(num_hidden_layers=3, num_attention_heads=2, num_key_value_heads=1, head_dim=128, seed=12),
}


def words():
    return [f"w{i}" for i in range(VOCAB - 2)]


def write_tokenizer(path: str) -> int:
    """Word-level tokenizer: ids 0..VOCAB-3 are words, VOCAB-2 <unk>, VOCAB-1 <|endoftext|> (appended to every text)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {w: i for i, w in enumerate(words())}
    vocab["<unk>"] = VOCAB - 2
    vocab["<|endoftext|>"] = VOCAB - 1
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.post_processor = processors.TemplateProcessing(single="$A <|endoftext|>", pair="$A <|endoftext|> $B <|endoftext|>",
                                                      special_tokens=[("<|endoftext|>", VOCAB - 1)])
    tk.save(path)
    return VOCAB - 1


def main():
    from transformers import Qwen3Config, Qwen3Model

    for name, spec in FIXTURES.items():
        spec = dict(spec)
        seed = spec.pop("seed")
        torch.manual_seed(seed)
        cfg = Qwen3Config(vocab_size=VOCAB, hidden_size=256, intermediate_size=128, max_position_embeddings=1024,
                          rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True, attention_bias=False,
                          torch_dtype="bfloat16", **spec)
        model = Qwen3Model(cfg).eval().to(torch.float32)
        with torch.no_grad():   # trained-model-like scales: norms around 1, not exactly 1
            for n, p in model.named_parameters():
                if n.endswith("norm.weight"):
                    p.copy_(1 + 0.1 * torch.randn_like(p))
        d = os.path.join(HERE, name)
        os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
        model.save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
        eos = write_tokenizer(os.path.join(d, "tokenizer.json"))
        with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": 256, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False,
                       "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
                       "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": True,
                       "include_prompt": True}, f, indent=2)
        with open(os.path.join(d, "config_sentence_transformers.json"), "w") as f:
            json.dump({"prompts": {"query": QUERY_PROMPT, "document": ""}, "default_prompt_name": None,
                       "similarity_fn_name": "cosine"}, f, indent=2)
        rng = np.random.default_rng(seed)
        seqs = [np.append(rng.integers(0, VOCAB - 2, n - 1), eos).astype(np.int32) for n in LENGTHS]
        embs = []
        with torch.no_grad():
            for s in seqs:
                h = model(input_ids=torch.from_numpy(s.astype(np.int64))[None]).last_hidden_state[0, -1]
                embs.append(torch.nn.functional.normalize(h, dim=0).numpy())
        np.savez_compressed(os.path.join(HERE, f"{name}_expected.npz"), ids=np.concatenate(seqs),
                            lens=np.asarray(LENGTHS, dtype=np.int32), emb=np.stack(embs).astype(np.float32))
        for root, _, files in os.walk(d):
            for fn in files:
                assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
        print(name, "written")


if __name__ == "__main__":
    main()
