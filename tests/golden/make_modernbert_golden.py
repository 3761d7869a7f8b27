"""Writes the ModernBERT fixtures under tests/golden/ (run on a machine with transformers; CPU):

  modernbert_cls_l4/, modernbert_mean_l5/   random ``ModernBertForSequenceClassification`` checkpoint directories (one label; hidden
                                  256, 4 heads of 64, intermediate_size 192, vocab 384, 1024 positions, ``local_attention`` 32:
                                  the window is +-16): config.json, sharded model.safetensors (every file under 1 MiB), a
                                  word-level tokenizer.json (templates ``[CLS] $A [SEP]`` / ``[CLS] $A [SEP] $B [SEP]``) and
                                  1_Pooling/config.json.  The first pools the [CLS] token and has 4 layers, global every 3rd
                                  (global, local, local, global); the second pools the mean and has 5 layers, global every 2nd,
                                  and names nomic-style prompts in config_sentence_transformers.json.
  modernbert_<dir>_expected.npz   ragged token-id inputs (flat ``ids`` + ``lens``) and, per sequence,
                                  ``logit_fp32``      the fp32 transformers model, one sequence per call (no padding enters),
                                  ``logit_bf16/fp16`` the same model with weights and activations cast to that type (each cast afresh
                                                      from the fp32 weights), run on the CPU,
                                  ``logit_allglobal`` fp32, the window switched off      } defect references; ``*_counted`` marks the
                                  ``logit_onetheta``  fp32, the global RoPE base everywhere } sequences where they differ from
                                  ``logit_nonorm``    fp32, the final norm left out         } ``logit_fp32`` by more than 4 e_ref[fp16]
                                  ``emb``             the pooled (as 1_Pooling says), L2-normalised final hidden states, fp32;
                                  plus ``pair_query`` / ``pair_passage`` strings and ``pair_logit`` (fp32, tokenised by the fixture
                                  tokenizer) for the surface test.

  modernbert_<dir>_hidden.npz     ``hidden_idx`` / ``hidden_<k>``: the final-normed hidden states of four of those sequences
                                  (17, 34, 129 and 600 tokens), fp32; ``hidden_e_bf16`` / ``hidden_e_fp16``: the largest deviation
                                  from them of the same model cast to that type (CPU).

    python tests/golden/make_modernbert_golden.py
"""
import copy
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB = 384
PAD, CLS, SEP, UNK, FIRST_WORD = 0, 1, 2, 3, 4
REQUIRED_LENGTHS = [1, 2, 15, 16, 17, 33, 34, 129, 257, 600]
FIXTURES = {
    "modernbert_cls_l4": dict(num_hidden_layers=4, global_attn_every_n_layers=3, classifier_pooling="cls", seed=31, qk_sharpen=6.0),
    "modernbert_mean_l5": dict(num_hidden_layers=5, global_attn_every_n_layers=2, classifier_pooling="mean", seed=32, qk_sharpen=12.0),
}
PAIRS = [("w5 w17 w3", "w99 w5 w200 w17 w31 w8 w3"), ("w5 w17 w3", "w300 w301 w12"), ("w1", "w2"),
         ("w40 w41 w42 w43 w44 w45", "w7"), ("w250 w9", " ".join(f"w{(7 * i) % 380}" for i in range(90))),
         (" ".join(f"w{(11 * i) % 380}" for i in range(40)), " ".join(f"w{(13 * i + 5) % 380}" for i in range(150)))]


def write_tokenizer(path: str) -> None:
    """Word-level tokenizer: [PAD] 0, [CLS] 1, [SEP] 2, [UNK] 3, then the words w0 .. w379."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {"[PAD]": PAD, "[CLS]": CLS, "[SEP]": SEP, "[UNK]": UNK}
    vocab.update({f"w{i}": FIRST_WORD + i for i in range(VOCAB - FIRST_WORD)})
    tk = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]",
                                                      special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    tk.save(path)


def sequences(rng):
    """>= 40 ragged sequences: the required lengths, and random ones of which most exceed the +-16 window."""
    lens = REQUIRED_LENGTHS + rng.integers(34, 400, 28).tolist() + rng.integers(3, 34, 6).tolist()
    return [rng.integers(0, VOCAB, n).astype(np.int32) for n in lens]


def variant(model, mutate):
    """A fresh model of the same weights under a config changed by ``mutate`` (masks and rotary tables are built from the config)."""
    from transformers import ModernBertForSequenceClassification

    cfg = copy.deepcopy(model.config)
    mutate(cfg)
    m = ModernBertForSequenceClassification(cfg).eval().to(torch.float32)
    m.load_state_dict(model.state_dict())
    return m


def main():
    from tokenizers import Tokenizer
    from transformers import ModernBertConfig, ModernBertForSequenceClassification

    for name, spec in FIXTURES.items():
        spec = dict(spec)
        # Q and K rows of Wqkv are scaled by qk_sharpen: peaked attention, so that window and RoPE base matter to the logit (the mean
        # over a sequence's tokens averages more of it away than the [CLS] row does)
        seed, qk_sharpen = spec.pop("seed"), spec.pop("qk_sharpen")
        torch.manual_seed(seed)
        cfg = ModernBertConfig(vocab_size=VOCAB, hidden_size=256, intermediate_size=192, num_attention_heads=4,
                               max_position_embeddings=1024, local_attention=32, num_labels=1, pad_token_id=PAD, bos_token_id=CLS,
                               eos_token_id=SEP, cls_token_id=CLS, sep_token_id=SEP, **spec)
        model = ModernBertForSequenceClassification(cfg).eval().to(torch.float32)
        rng = np.random.default_rng(seed)
        seqs = sequences(rng)
        lens = [len(s) for s in seqs]
        assert len(seqs) >= 40 and set(REQUIRED_LENGTHS) <= set(lens) and sum(n > 33 for n in lens) >= 30

        def logits_of(m, tokens):
            with torch.no_grad():
                return np.asarray([float(m(input_ids=torch.from_numpy(s.astype(np.int64))[None]).logits[0, 0]) for s in tokens])

        with torch.no_grad():
            for n, p in model.named_parameters():   # trained-model-like scales: norms around 1, not exactly 1
                if n.endswith("norm.weight"):
                    p.copy_(1 + 0.1 * torch.randn_like(p))
            # Embedding(padding_idx=) zeroed this row; trained checkpoints carry ordinary values there
            model.model.embeddings.tok_embeddings.weight[PAD].copy_(0.02 * torch.randn(cfg.hidden_size))
            for layer in model.model.layers:
                layer.attn.Wqkv.weight[: 2 * cfg.hidden_size].mul_(qk_sharpen)
            # a head at the init scale gives CLS logits bunched within 0.4 of each other, scores that test nothing: widen the
            # head and the classifier until the asserted span of scores holds
            model.head.dense.weight.copy_(0.05 * torch.randn_like(model.head.dense.weight))
            model.classifier.weight.copy_(0.15 * torch.randn_like(model.classifier.weight))
            model.classifier.bias.zero_()
            for _ in range(40):
                fp32 = logits_of(model, seqs)
                score = 1 / (1 + np.exp(-fp32))
                if score.min() < 0.1 and score.max() > 0.9:
                    break
                model.classifier.weight.mul_(1.5)
                model.classifier.bias.copy_(-torch.tensor(float(np.median(fp32))) * 1.5 + model.classifier.bias * 1.5)
        fp32 = logits_of(model, seqs)
        score = 1 / (1 + np.exp(-fp32))
        assert score.min() < 0.1 and score.max() > 0.9, (score.min(), score.max())

        sd = model.state_dict()
        assert sorted(k for k in sd if not k.startswith("model.")) == ["classifier.bias", "classifier.weight", "head.dense.weight",
                                                                      "head.norm.weight"]
        assert "model.layers.0.attn_norm.weight" not in sd and "model.layers.1.attn_norm.weight" in sd
        d = os.path.join(HERE, name)
        os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
        model.save_pretrained(d, max_shard_size="900KB", safe_serialization=True)
        write_tokenizer(os.path.join(d, "tokenizer.json"))
        pooling = spec["classifier_pooling"]
        with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": 256, "pooling_mode_cls_token": pooling == "cls",
                       "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False,
                       "pooling_mode_mean_sqrt_len_tokens": False, "pooling_mode_weightedmean_tokens": False,
                       "pooling_mode_lasttoken": False, "include_prompt": True}, f, indent=2)
        if pooling == "mean":
            with open(os.path.join(d, "config_sentence_transformers.json"), "w") as f:
                json.dump({"prompts": {"query": "search_query: ", "document": "search_document: "}, "default_prompt_name": None,
                           "similarity_fn_name": "cosine"}, f, indent=2)
        with open(os.path.join(d, "config.json")) as f:
            saved = json.load(f)
        every = spec["global_attn_every_n_layers"]
        assert saved["architectures"] == ["ModernBertForSequenceClassification"] and saved["model_type"] == "modernbert"
        assert saved["layer_types"] == ["full_attention" if i % every == 0 else "sliding_attention" for i in range(cfg.num_hidden_layers)]
        assert saved["rope_parameters"]["full_attention"]["rope_theta"] == 160000.0
        assert saved["rope_parameters"]["sliding_attention"]["rope_theta"] == 10000.0

        low = {}
        for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            low[key] = logits_of(copy.deepcopy(model).to(dt), seqs)      # cast afresh from the fp32 weights
        e_ref = {k: float(np.abs(v - fp32).max()) for k, v in low.items()}

        # defect references, and the separation the GPU test relies on: asserted here
        def one_theta(c):
            c.rope_parameters = {k: dict(v, rope_theta=c.rope_parameters["full_attention"]["rope_theta"])
                                 for k, v in c.rope_parameters.items()}

        def no_window(c):
            c.local_attention = 4096

        nonorm_model = copy.deepcopy(model)
        nonorm_model.model.final_norm = torch.nn.Identity()
        defects = {"allglobal": logits_of(variant(model, no_window), seqs), "onetheta": logits_of(variant(model, one_theta), seqs),
                   "nonorm": logits_of(nonorm_model, seqs)}
        counted = {k: np.abs(v - fp32) > 4 * e_ref["fp16"] for k, v in defects.items()}
        for k, c in counted.items():
            assert c.sum() >= 10, f"{name}: defect '{k}' separates only {int(c.sum())} sequences by 4 e_ref[fp16] = {4 * e_ref['fp16']:.5f}"
        # the window rule itself: a sequence inside the window is untouched by switching it off
        short = np.asarray(lens) <= 17
        assert np.abs(defects["allglobal"] - fp32)[short].max() < 1e-5

        hidden_idx = [lens.index(17), lens.index(34), lens.index(129), lens.index(600)]
        embs, hidden = [], {}
        with torch.no_grad():
            for i, s in enumerate(seqs):
                h = model.model(input_ids=torch.from_numpy(s.astype(np.int64))[None]).last_hidden_state[0]
                p = h[0] if pooling == "cls" else h.mean(0)
                embs.append(torch.nn.functional.normalize(p, dim=0).numpy())
                if i in hidden_idx:
                    hidden[f"hidden_{hidden_idx.index(i)}"] = h.numpy().astype(np.float32)

        # the reference's own 16-bit error on those hidden states (the bound of the GPU test, like e_ref of the logits)
        hidden_e = {}
        for key, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            m16 = copy.deepcopy(model).to(dt)
            with torch.no_grad():
                hidden_e[f"hidden_e_{key}"] = max(
                    float((m16.model(input_ids=torch.from_numpy(seqs[i].astype(np.int64))[None]).last_hidden_state[0].float()
                           - torch.from_numpy(hidden[f"hidden_{k}"])).abs().max()) for k, i in enumerate(hidden_idx))

        tk = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
        pair_ids = [np.asarray(tk.encode(q, p).ids, dtype=np.int32) for q, p in PAIRS]
        assert all(i[0] == CLS and i[-1] == SEP and (i == SEP).sum() == 2 and UNK not in i for i in pair_ids)
        np.savez_compressed(
            os.path.join(HERE, f"{name}_expected.npz"), ids=np.concatenate(seqs), lens=np.asarray(lens, dtype=np.int32),
            logit_fp32=fp32.astype(np.float64), logit_bf16=low["bf16"].astype(np.float64), logit_fp16=low["fp16"].astype(np.float64),
            logit_allglobal=defects["allglobal"], logit_onetheta=defects["onetheta"], logit_nonorm=defects["nonorm"],
            allglobal_counted=counted["allglobal"], onetheta_counted=counted["onetheta"], nonorm_counted=counted["nonorm"],
            emb=np.stack(embs).astype(np.float32),
            pair_query=np.asarray([q for q, _ in PAIRS]), pair_passage=np.asarray([p for _, p in PAIRS]),
            pair_logit=logits_of(model, pair_ids).astype(np.float64))
        np.savez_compressed(os.path.join(HERE, f"{name}_hidden.npz"), hidden_idx=np.asarray(hidden_idx, dtype=np.int32), **hidden,
                            **{k: np.float64(v) for k, v in hidden_e.items()})
        assert os.path.getsize(os.path.join(HERE, f"{name}_hidden.npz")) < 1 << 20
        for root, _, files in os.walk(d):
            for fn in files:
                assert os.path.getsize(os.path.join(root, fn)) < 1 << 20, fn
        assert os.path.getsize(os.path.join(HERE, f"{name}_expected.npz")) < 1 << 20
        print(name, "written:", len(seqs), "sequences, fp32 logits", fp32.min(), "..", fp32.max(), "e_ref", e_ref,
              "hidden e_ref", hidden_e, "counted", {k: int(c.sum()) for k, c in counted.items()},
              "defect shifts", {k: (float(np.abs(v - fp32).min()), float(np.abs(v - fp32).max())) for k, v in defects.items()})


if __name__ == "__main__":
    main()
