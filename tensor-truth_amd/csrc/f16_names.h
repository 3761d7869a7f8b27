// External names of the fp16 instantiation of gemm.hip / attention.hip / rowops.hip / encoder_api.hip (common.h, TT_F16).
#pragma once
// launch functions (encoder.h)
#define tt_gemm_launch tt_gemm_launch_f16
#define tt_scan_gemm_launch tt_scan_gemm_launch_f16
#define tt_scan_gemm_sample_launch tt_scan_gemm_sample_launch_f16
#define tt_gemm_skinny_enabled tt_gemm_skinny_enabled_f16
#define tt_attention_launch tt_attention_launch_f16
#define tt_attention_cls_launch tt_attention_cls_launch_f16
#define tt_attention_keylimit_launch tt_attention_keylimit_launch_f16
#define tt_absmax_launch tt_absmax_launch_f16
#define tt_embed_ln_launch tt_embed_ln_launch_f16
#define tt_layernorm_launch tt_layernorm_launch_f16
#define tt_gather_rows_launch tt_gather_rows_launch_f16
#define tt_quantize_rows_launch tt_quantize_rows_launch_f16
#define tt_adjacent_cosine_launch tt_adjacent_cosine_launch_f16
#define tt_cls_pool_l2norm_launch tt_cls_pool_l2norm_launch_f16
#define tt_head_out_sigmoid_launch tt_head_out_sigmoid_launch_f16
#define tt_mean_pool_l2norm_launch tt_mean_pool_l2norm_launch_f16
// C ABI (include/tt_hip.h declares the _f16 names)
#define tt_encoder_workspace_bytes tt_encoder_workspace_bytes_f16
#define tt_encoder_cls_workspace_bytes tt_encoder_cls_workspace_bytes_f16
#define tt_encoder_forward tt_encoder_forward_f16
#define tt_encoder_forward_cls tt_encoder_forward_cls_f16
#define tt_encoder_forward_keylen tt_encoder_forward_keylen_f16
#define tt_embed_pool tt_embed_pool_f16
#define tt_embed_pool_mean tt_embed_pool_mean_f16
#define tt_rerank_head tt_rerank_head_f16
#define tt_gemm_bf16 tt_gemm_f16
#define tt_layernorm_bf16 tt_layernorm_f16
#define tt_attention_varlen tt_attention_varlen_f16
// x3_path.hip a second time: the split planes are fp16 there ("f16x3": 22 significand bits per operand instead of bf16x3's 16 --
// down to fp16's subnormal grid: |x - hi - lo| <= max(2^-22 |x|, 2^-25), and nothing beyond +-65504)
#define tt_encoder_x3_workspace_bytes tt_encoder_x3_workspace_bytes_f16
#define tt_encoder_x3_cls_workspace_bytes tt_encoder_x3_cls_workspace_bytes_f16
#define tt_encoder_forward_x3 tt_encoder_forward_x3_f16
#define tt_encoder_forward_x3_cls tt_encoder_forward_x3_cls_f16
#define tt_rerank_head_x3 tt_rerank_head_x3_f16
#define tt_split_planes tt_split_planes_f16
#define tt_gemm_x3 tt_gemm_x3_f16
#define tt_gemm_x3_ex tt_gemm_x3_ex_f16
#define tt_attention_x3 tt_attention_x3_f16
#define tt_attention_x3_hd tt_attention_x3_hd_f16
#define tt_attention_cls_varlen tt_attention_cls_varlen_f16
// decoder.hip a second time: the decoder embedder in fp16
#define tt_decoder_workspace_bytes tt_decoder_workspace_bytes_f16
#define tt_decoder_forward tt_decoder_forward_f16
#define tt_decoder_rows_workspace_bytes tt_decoder_rows_workspace_bytes_f16
#define tt_decoder_forward_rows tt_decoder_forward_rows_f16
#define tt_decoder_score tt_decoder_score_f16
#define tt_embed_pool_last tt_embed_pool_last_f16
#define tt_attention_causal_gqa tt_attention_causal_gqa_f16
#define tt_qk_norm_rope tt_qk_norm_rope_f16
// modernbert.hip a second time: the ModernBERT encoders in fp16
#define tt_modernbert_workspace_bytes tt_modernbert_workspace_bytes_f16
#define tt_modernbert_forward tt_modernbert_forward_f16
#define tt_modernbert_head tt_modernbert_head_f16
#define tt_rope_v8 tt_rope_v8_f16
#define tt_attention_window tt_attention_window_f16
// mpnet.hip a second time: the MPNet encoders in fp16
#define tt_mpnet_workspace_bytes tt_mpnet_workspace_bytes_f16
#define tt_mpnet_forward tt_mpnet_forward_f16
#define tt_attention_relbias tt_attention_relbias_f16
// deberta.hip a second time: the DeBERTa-v2 / v3 cross-encoders in fp16
#define tt_deberta_workspace_bytes tt_deberta_workspace_bytes_f16
#define tt_deberta_forward tt_deberta_forward_f16
#define tt_deberta_head tt_deberta_head_f16
#define tt_attention_disentangled tt_attention_disentangled_f16
// ropebert.hip a second time: the NomicBERT / Jina-v3 encoders in fp16
#define tt_ropebert_workspace_bytes tt_ropebert_workspace_bytes_f16
#define tt_ropebert_forward tt_ropebert_forward_f16
// jinabert.hip a second time: the JinaBERT (jina-embeddings-v2) encoders in fp16
#define tt_jinabert_workspace_bytes tt_jinabert_workspace_bytes_f16
#define tt_jinabert_forward tt_jinabert_forward_f16
#define tt_attention_alibi tt_attention_alibi_f16
// colbert.hip a second time: late-interaction scoring, projection and key-limited attention in fp16
#define tt_maxsim tt_maxsim_f16
#define tt_maxsim_scan_topk tt_maxsim_scan_topk_f16
#define tt_colbert_project tt_colbert_project_f16
#define tt_attention_keylimit tt_attention_keylimit_f16
// lexical.hip a second time: the lexical weights of an fp16 hidden state (the scores are fp32 / bf16 by definition: compiled once)
#define tt_lexical_weights tt_lexical_weights_f16
// multivec.hip a second time: the wide projection and the wide MaxSim on fp16 vectors (the _f32 projection and the mix: compiled once)
#define tt_multivec_project tt_multivec_project_f16
#define tt_maxsim_wide tt_maxsim_wide_f16
// splade.hip a second time: the vocabulary projection with its segmented maximum on fp16 operands (the compaction is fp32: compiled once)
#define tt_splade_pool tt_splade_pool_f16
