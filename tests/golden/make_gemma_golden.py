"""Writes the EmbeddingGemma fixture under tests/golden/ (run on a machine with transformers 5.x; CPU):

  gemma_mean_l5/                a random bidirectional ``Gemma3TextModel`` checkpoint directory in the layout of
                                google/embeddinggemma-300m (hidden 256, 2 query heads over 1 KV head of 256, intermediate_size 192,
                                vocab 384, 1024 positions, 5 layers: sliding, sliding, full, sliding, full; window +-16): config.json,
                                sharded model.safetensors in bf16 (every file under 1 MiB), a word-level tokenizer.json (template
                                ``[BOS] $A [EOS]``), modules.json, 1_Pooling/ (mean), 2_Dense/ (256 -> 512) and 3_Dense/ (512 -> 256;
                                no bias, identity activation, fp32 ``linear.weight``), and config_sentence_transformers.json with the
                                "query" and "document" prompts.
  gemma_mean_l5_expected.npz    ragged token-id inputs (flat ``ids`` + ``lens``) and, per sequence (one sequence per call: no padding
                                enters), every value from the model LOADED BACK from that directory -- transformers rewrites a
                                bidirectional config's ``sliding_window`` S to S // 2 + 1 on every load and ``save_pretrained`` writes
                                the rewritten value, so only the reloaded model agrees with the file:
                                ``emb_fp32``       the fp32 model's embedding,
                                ``emb_bf16``       the same model and tail cast to bf16, run on the CPU,
                                ``e_ref``          max |emb_bf16 - emb_fp32| over all sequences and components,
                                ``emb_nowindow``   fp32, the window switched off, RoPE bases unchanged     } defect references;
                                ``emb_onetheta``   fp32, the global RoPE base everywhere                   } ``*_counted`` marks the
                                ``emb_causal``     fp32, ``use_bidirectional_attention`` false             } sequences where they
                                ``emb_plainnorm``  fp32, the norms computed with w instead of 1 + w        } differ from ``emb_fp32``
                                ``emb_nodense``    fp32, mean then normalise, without the Dense pair       } by more than 4 e_ref
                                plus ``text`` strings with ``text_query_emb`` / ``text_document_emb``: the fp32 embeddings of
                                prompt + text through the fixture tokenizer.
  gemma_mean_l5_hidden.npz      ``hidden_idx`` / ``hidden_<k>``: the final-normed hidden states of four of those sequences (17, 34,
                                129 and 600 tokens), fp32; ``hidden_e_bf16``: the largest deviation from them of the bf16 model (CPU).

sentence-transformers is not installed where this runs: its four modules behind the transformer -- ``Pooling`` (mean over the
sequence's tokens), ``Dense`` (``linear(x)``, no bias, identity activation) twice, ``Normalize`` (x / max(||x||_2, 1e-12)) -- are
restated in torch below (``tail``); with one unpadded sequence per call the attention mask of ``Pooling`` is all ones.

    python tests/golden/make_gemma_golden.py
"""
import copy
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "gemma_mean_l5"
VOCAB = 384
PAD, BOS, EOS, UNK, FIRST_WORD = 0, 1, 2, 3, 4
PROMPT_WORDS = ["task:", "search", "result", "|", "query:", "title:", "none", "text:"]
PROMPTS = {"query": "task: search result | query: ", "document": "title: none | text: "}
N_WORDS = VOCAB - FIRST_WORD - len(PROMPT_WORDS)
REQUIRED_LENGTHS = [1, 2, 15, 16, 17, 33, 34, 129, 257, 600]
LAYER_TYPES = ["sliding_attention", "sliding_attention", "full_attention", "sliding_attention", "full_attention"]
HIDDEN, DENSE = 256, 512
WINDOW = 16                       # the effective window: |q - k| <= 16
SEED = 41
TEXTS = ["w5 w17 w3", "w300 w301 w12", "w1", " ".join(f"w{(7 * i) % N_WORDS}" for i in range(90)),
         " ".join(f"w{(13 * i + 5) % N_WORDS}" for i in range(150))]


def write_tokenizer(path: str) -> None:
    """Word-level tokenizer: [PAD] 0, [BOS] 1, [EOS] 2, [UNK] 3, the words w0 .. w371, then the words of the two prompts."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {"[PAD]": PAD, "[BOS]": BOS, "[EOS]": EOS, "[UNK]": UNK}
    vocab.update({f"w{i}": FIRST_WORD + i for i in range(N_WORDS)})
    vocab.update({w: FIRST_WORD + N_WORDS + i for i, w in enumerate(PROMPT_WORDS)})
    assert len(vocab) == VOCAB
    tk = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.post_processor = processors.TemplateProcessing(single="[BOS] $A [EOS]", pair="[BOS] $A [EOS] $B [EOS]",
                                                      special_tokens=[("[BOS]", BOS), ("[EOS]", EOS)])
    tk.save(path)


def sequences(rng):
    """44 ragged sequences: the required lengths, 28 beyond the +-16 window's reach and 6 short ones."""
    lens = REQUIRED_LENGTHS + rng.integers(34, 401, 28).tolist() + rng.integers(3, 35, 6).tolist()
    return [rng.integers(0, VOCAB, n).astype(np.int32) for n in lens]


def variant(model, mutate):
    """A fresh fp32 model of the same weights under a config changed by ``mutate`` (masks and rotary tables are built from the
    config; a config object handed to the constructor is not rewritten again)."""
    from transformers import Gemma3TextModel

    cfg = copy.deepcopy(model.config)
    mutate(cfg)
    m = Gemma3TextModel(cfg).eval().to(torch.float32)
    m.load_state_dict(model.state_dict())
    return m


def tail(h, dense, dtype=torch.float32):
    """sentence-transformers Pooling(mean) -> Dense -> Dense -> Normalize of one sequence's hidden states h [n][H], in ``dtype``."""
    p = h.to(dtype).sum(0) / torch.tensor(float(h.shape[0]), dtype=dtype)
    for w in dense:
        p = torch.nn.functional.linear(p, w.to(dtype))
    return torch.nn.functional.normalize(p, p=2, dim=0)


def build(qk_sharpen: float, d: str):
    """Draw the model, write the checkpoint directory ``d`` and -> (the fp32 model loaded back from it, the Dense pair)."""
    from safetensors.torch import save_file
    from transformers import Gemma3TextConfig, Gemma3TextModel

    torch.manual_seed(SEED)
    # transformers rewrites sliding_window S to S // 2 + 1 here, and once more when the written directory is loaded:
    # 65 -> 33 (written) -> 17 (loaded): |q - k| < 17, i.e. config.json's 33 means |q - k| <= 33 // 2 = 16
    cfg = Gemma3TextConfig(vocab_size=VOCAB, hidden_size=HIDDEN, intermediate_size=192, num_hidden_layers=5, num_attention_heads=2,
                           num_key_value_heads=1, head_dim=256, max_position_embeddings=1024, sliding_window=4 * WINDOW + 1,
                           layer_types=list(LAYER_TYPES), use_bidirectional_attention=True, query_pre_attn_scalar=256,
                           rms_norm_eps=1e-6, pad_token_id=PAD, bos_token_id=BOS, eos_token_id=EOS)
    assert cfg.sliding_window == 2 * WINDOW + 1
    model = Gemma3TextModel(cfg).eval().to(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("norm.weight"):           # (1 + w) norms: a zero-initialised w would test nothing
                p.copy_(0.3 * torch.randn_like(p))
        # Embedding(padding_idx=) zeroed this row; trained checkpoints carry ordinary values there
        model.embed_tokens.weight[PAD].copy_(0.02 * torch.randn(HIDDEN))
        for layer in model.layers:                  # peaked attention, so that window, RoPE base and mask matter to the embedding
            layer.self_attn.q_proj.weight.mul_(qk_sharpen)
            layer.self_attn.k_proj.weight.mul_(qk_sharpen)
    dense = [0.06 * torch.randn(DENSE, HIDDEN), 0.05 * torch.randn(HIDDEN, DENSE)]

    for sub in ("1_Pooling", "2_Dense", "3_Dense"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    for fn in os.listdir(d):                        # shards of an earlier run with another shard count
        if fn.endswith(".safetensors") or fn.endswith(".index.json"):
            os.remove(os.path.join(d, fn))
    model.to(torch.bfloat16).save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
    write_tokenizer(os.path.join(d, "tokenizer.json"))
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Dense", "type": "sentence_transformers.models.Dense"},
                   {"idx": 3, "name": "3", "path": "3_Dense", "type": "sentence_transformers.models.Dense"},
                   {"idx": 4, "name": "4", "path": "4_Normalize", "type": "sentence_transformers.models.Normalize"}], f, indent=2)
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": HIDDEN, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
                   "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
                   "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": False, "include_prompt": True}, f, indent=2)
    for sub, w in zip(("2_Dense", "3_Dense"), dense):
        with open(os.path.join(d, sub, "config.json"), "w") as f:
            json.dump({"in_features": w.shape[1], "out_features": w.shape[0], "bias": False,
                       "activation_function": "torch.nn.modules.linear.Identity"}, f, indent=2)
        save_file({"linear.weight": w.contiguous()}, os.path.join(d, sub, "model.safetensors"))
    with open(os.path.join(d, "config_sentence_transformers.json"), "w") as f:
        json.dump({"prompts": PROMPTS, "default_prompt_name": None, "similarity_fn_name": "cosine"}, f, indent=2)

    with open(os.path.join(d, "config.json")) as f:
        saved = json.load(f)
    assert saved["model_type"] == "gemma3_text" and saved["use_bidirectional_attention"] is True
    assert saved["sliding_window"] == 2 * WINDOW + 1 and saved["sliding_window"] // 2 == WINDOW
    assert saved["layer_types"] == LAYER_TYPES and saved["query_pre_attn_scalar"] == saved["head_dim"] == 256
    assert saved["rope_parameters"]["full_attention"]["rope_theta"] == 1e6
    assert saved["rope_parameters"]["sliding_attention"]["rope_theta"] == 1e4
    loaded = Gemma3TextModel.from_pretrained(d, dtype=torch.float32).eval()
    assert loaded.config.sliding_window == WINDOW + 1 and loaded.config.use_bidirectional_attention
    assert loaded.embed_tokens.weight.dtype == torch.float32
    return loaded, dense


def main():
    from tokenizers import Tokenizer

    d = os.path.join(HERE, NAME)
    rng = np.random.default_rng(SEED)
    seqs = sequences(rng)
    lens = [len(s) for s in seqs]
    assert len(seqs) >= 40 and set(REQUIRED_LENGTHS) <= set(lens)

    def hidden_of(m, s):
        with torch.no_grad():
            return m(input_ids=torch.from_numpy(np.asarray(s, dtype=np.int64))[None]).last_hidden_state[0]

    def embs_of(m, tokens, dense, dtype=torch.float32):
        return np.stack([tail(hidden_of(m, s), dense, dtype).float().numpy() for s in tokens])

    for qk_sharpen in (6.0, 9.0, 12.0, 16.0, 24.0):
        model, dense = build(qk_sharpen, d)
        fp32 = embs_of(model, seqs, dense)
        bf16 = embs_of(copy.deepcopy(model).to(torch.bfloat16), seqs, dense, torch.bfloat16)
        e_ref = float(np.abs(bf16 - fp32).max())

        def no_window(c):
            c.sliding_window = 4096

        def one_theta(c):
            c.rope_parameters = {k: dict(v, rope_theta=c.rope_parameters["full_attention"]["rope_theta"])
                                 for k, v in c.rope_parameters.items()}

        def causal(c):
            c.use_bidirectional_attention = False

        plain = copy.deepcopy(model)
        with torch.no_grad():
            for n, p in plain.named_parameters():
                if n.endswith("norm.weight"):
                    p.sub_(1.0)                     # 1 + (w - 1) = w
        defects = {"nowindow": embs_of(variant(model, no_window), seqs, dense), "onetheta": embs_of(variant(model, one_theta), seqs, dense),
                   "causal": embs_of(variant(model, causal), seqs, dense), "plainnorm": embs_of(plain, seqs, dense),
                   "nodense": embs_of(model, seqs, [])}
        counted = {k: np.abs(v - fp32).max(1) > 4 * e_ref for k, v in defects.items()}
        print(f"qk_sharpen {qk_sharpen}: e_ref {e_ref:.5f}; counted", {k: int(c.sum()) for k, c in counted.items()})
        if all(c.sum() >= 20 for c in counted.values()):
            break
    for k, c in counted.items():
        assert c.sum() >= 20, f"defect '{k}' separates only {int(c.sum())} sequences by 4 e_ref = {4 * e_ref:.5f}"
    # the window rule itself: a sequence inside the window is untouched by switching it off, one a token longer is not
    short = np.asarray(lens) <= WINDOW + 1
    assert np.abs(defects["nowindow"] - fp32)[short].max() < 1e-5

    hidden_idx = [lens.index(n) for n in (17, 34, 129, 600)]
    hidden = {f"hidden_{k}": hidden_of(model, seqs[i]).numpy().astype(np.float32) for k, i in enumerate(hidden_idx)}
    m16 = copy.deepcopy(model).to(torch.bfloat16)
    hidden_e = max(float((hidden_of(m16, seqs[i]).float() - torch.from_numpy(hidden[f"hidden_{k}"])).abs().max())
                   for k, i in enumerate(hidden_idx))

    tk = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
    text_emb = {}
    for kind, prompt in PROMPTS.items():
        ids = [np.asarray(tk.encode(prompt + t).ids, dtype=np.int32) for t in TEXTS]
        assert all(i[0] == BOS and i[-1] == EOS and UNK not in i for i in ids)
        text_emb[kind] = embs_of(model, ids, dense)

    np.savez_compressed(
        os.path.join(HERE, f"{NAME}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(lens, dtype=np.int32),
        emb_fp32=fp32.astype(np.float32), emb_bf16=bf16.astype(np.float32), e_ref=np.float64(e_ref),
        **{f"emb_{k}": v.astype(np.float32) for k, v in defects.items()}, **{f"{k}_counted": c for k, c in counted.items()},
        text=np.asarray(TEXTS), text_query_emb=text_emb["query"].astype(np.float32),
        text_document_emb=text_emb["document"].astype(np.float32), qk_sharpen=np.float64(qk_sharpen))
    np.savez_compressed(os.path.join(HERE, f"{NAME}_hidden.npz"), hidden_idx=np.asarray(hidden_idx, dtype=np.int32), **hidden,
                        hidden_e_bf16=np.float64(hidden_e))
    for root, _, files in os.walk(d):
        for fn in files:
            assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
    for fn in (f"{NAME}_expected.npz", f"{NAME}_hidden.npz"):
        assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn
    print(NAME, "written:", len(seqs), "sequences, qk_sharpen", qk_sharpen, "e_ref", e_ref, "hidden e_ref", hidden_e, "counted",
          {k: int(c.sum()) for k, c in counted.items()},
          "defect shifts", {k: (float(np.abs(v - fp32).max(1).min()), float(np.abs(v - fp32).max())) for k, v in defects.items()})


if __name__ == "__main__":
    main()
