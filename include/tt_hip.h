/* tt_hip.h -- C ABI of libtt_hip.so, the MI355X (gfx950) implementation of
 * tensor-truth's retrieval hot path (embed -> exact top-k scan -> rerank).
 *
 * The reference (ljubobratovicrelja/tensor-truth) is pure Python and has no FFI
 * for this path; its "plugin boundary" is three LlamaIndex interfaces (SURVEY.md
 * section 8b).  Each entry point below names the reference call site whose
 * arithmetic it replaces.  The Python classes in tensor_truth_amd/ mirror the
 * reference's interfaces and call these functions through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - the caller owns all buffers (torch tensors); nothing is allocated or freed
 *     inside a launch function, nothing synchronises the device, so every call
 *     is stream-ordered and graph-capturable;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return 0 on success, a negative TT_E_* code on failure;
 *     tt_last_error() returns a thread-local message for the last failure;
 *   - re-entrant: no global mutable state, safe to call from the reference's
 *     executor threads (rag_engine.py:420-424) on distinct streams/workspaces;
 *   - bf16 tensors are raw uint16 storage, row-major, 16-byte aligned.
 */
#ifndef TT_HIP_H
#define TT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the declarations of this header -- and nothing else -- are its dynamic
 * symbols (`nm -D libtt_hip.so`; tests/test_lib_abi.py). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define TT_OK 0
#define TT_E_INVALID (-1)   /* bad argument (shape, alignment, null pointer)  */
#define TT_E_UNSUPPORTED (-2) /* shape outside the compiled kernel set         */
#define TT_E_WORKSPACE (-3) /* workspace too small                            */
#define TT_E_HIP (-4)       /* a HIP runtime call failed                      */

/* ---- library info ------------------------------------------------------- */
int tt_version(void);              /* ABI version, currently 1                */
const char* tt_arch(void);         /* "gfx950"                                */
const char* tt_last_error(void);   /* thread-local, never NULL                */
int tt_device_cu_count(void);      /* compute units of the current device, <0 on error */

/* ---- similarity scan + top-k --------------------------------------------
 * Replaces the vector search inside VectorIndexRetriever.retrieve
 * (reference: src/tensortruth/rag_engine.py:639,674 -> ChromaVectorStore.query,
 * collection created at rag_engine.py:628-630; upstream HNSW is approximate,
 * this is the exact scan BASELINE.json specifies):
 *     S[q][n] = sum_d Q[q][d] * C[n][d]      bf16 inputs, fp32 accumulate
 *     out = top-k per query by (score desc, row index asc)
 * Fewer than k valid rows -> trailing entries are (score -inf, index -1).
 * `dim` must be a multiple of 128 and <= 1024; 1 <= k <= 1024.
 * out_idx[q][j] = idx_base + local row index.
 * status_flag (device int32, may be NULL): set non-zero iff a candidate buffer
 * overflowed, in which case results for this call are NOT exact and the caller
 * must re-run through tt_scan_topk_exact (adversarial score distributions only).
 */
size_t tt_scan_workspace_bytes(int64_t n_rows, int dim, int n_queries, int k);

int tt_scan_topk(const void* corpus_bf16, int64_t n_rows, int dim,
                 const void* queries_bf16, int n_queries, int k, int32_t idx_base,
                 float* out_scores, int32_t* out_idx,
                 void* workspace, size_t workspace_bytes,
                 int32_t* status_flag, void* stream);

/* Always-exact variant: dense scores for every row + selection.  Needs
 * n_queries * n_rows * 4 bytes of workspace; meant for small shards and as the
 * overflow fallback. */
size_t tt_scan_exact_workspace_bytes(int64_t n_rows, int dim, int n_queries, int k);
int tt_scan_topk_exact(const void* corpus_bf16, int64_t n_rows, int dim,
                       const void* queries_bf16, int n_queries, int k, int32_t idx_base,
                       float* out_scores, int32_t* out_idx,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Segmented variant for several index modules living in ONE matrix (replaces the thread-pool fan-out
 * over per-module retrievers, src/tensortruth/rag_engine.py:420-424, and the n_indexes separate vector
 * searches behind it): rows [seg_offsets[s], seg_offsets[s+1]) are module s (host array of
 * n_segments + 1 non-decreasing offsets within [0, n_rows], 1 <= n_segments <= 64).  One pass over the
 * matrix scores every row once; every (query, segment) then gets its own exact top-k, ordered by
 * (score desc, row asc):  out_scores / out_idx are [n_queries][n_segments][k], indices are
 * SEGMENT-LOCAL rows, short or empty segments are padded with (-inf, -1).
 * Workspace: n_queries * rows * 4 bytes -- meant for the handful of queries of an
 * interactive retrieve(); large query batches over one big index go through tt_scan_topk. */
size_t tt_scan_segmented_workspace_bytes(int64_t n_rows, int dim, int n_queries, int k);
int tt_scan_topk_segmented(const void* corpus_bf16, int64_t n_rows, int dim,
                           const void* queries_bf16, int n_queries, int k,
                           const int64_t* seg_offsets, int n_segments,
                           float* out_scores, int32_t* out_idx,
                           void* workspace, size_t workspace_bytes, void* stream);

/* fp8 shadow of the corpus: an EXACT prefilter for the scan of a lone caller (the reference's own usage: one un-batched
 * retrieve() per query, src/tensortruth/rag_engine.py:420-424, README.md:13), where tt_scan_topk is one full read of the bf16
 * matrix (20.5 GB at 10 M x 1024: 3 ms).  The shadow block holds, for a capacity of cap_rows rows, the rows as e4m3 bytes
 * (x 256) and two floats per row -- be, the norm of what the rounding took, and dn, the norm of what it kept -- so that
 * with d = shadow / 256 and the bf16 query q itself, q.c <= q.d + ||q|| be bounds every row's exact score from above, and
 * 2 D 2^-23 ||q|| (dn + be) covers the fp32 accumulation of both passes (csrc/shadow.hip).
 * tt_scan_topk_shadow: threshold = k-th best exact score of a row sample (as tt_scan_topk); one pass over the SHADOW lists
 * the rows whose bound reaches it; those rows are re-scored from the bf16 matrix with tt_scan_topk's own arithmetic and the
 * same exact selection.  Scores and indices are bit-identical to tt_scan_topk's.  n_queries <= 4; rows [0, n_rows) of the
 * shadow must have been built from the same corpus rows (tt_scan_shadow_build, any sub-range at a time: appended rows only
 * need their own range).  status_flag as in tt_scan_topk (a survivor list that overflowed: re-run tt_scan_topk). */
size_t tt_scan_shadow_bytes(int64_t cap_rows, int dim);
int tt_scan_shadow_build(const void* corpus_bf16, int dim, int64_t row_lo, int64_t row_hi,
                         void* shadow, int64_t cap_rows, void* stream);
size_t tt_scan_shadow_workspace_bytes(int64_t n_rows, int dim, int n_queries, int k);
int tt_scan_topk_shadow(const void* corpus_bf16, const void* shadow, int64_t cap_rows, int64_t n_rows, int dim,
                        const void* queries_bf16, int n_queries, int k, int32_t idx_base,
                        float* out_scores, int32_t* out_idx,
                        void* workspace, size_t workspace_bytes, int32_t* status_flag, void* stream);

/* ---- MMR: diversified top-k over the scan's hits (csrc/mmr.hip) -----------------
 * Replaces the vector store's query mode "mmr" (index.as_retriever(vector_store_query_mode="mmr", ...): maximal marginal
 * relevance, Carbonell & Goldstein 1998) for the dense path: of the P best rows of a scan, pick k one at a time, each the
 * candidate that is most relevant AND least similar to what has been picked.
 *
 * tt_mmr_select: cand / rel are [n_queries][n_cand] (1 <= n_cand <= 1024), tt_scan_topk's out_idx / out_scores untouched: list
 *   entries in the scan's order (score descending, row ascending), corpus row = entry - idx_base, entries < 0 are padding, and an
 *   entry whose row falls outside [0, n_rows) is treated as padding too -- no row outside the matrix is read.
 *   Similarity: G[i][j] = the fp32 dot product of the bf16 corpus rows of list positions i and j: ONE mfma_f32_16x16x32_bf16 chain
 *   over kk = 0 .. dim/32 - 1 from a zero accumulator (the scan's and tt_maxsim's convention: unit rows, so the dot product is the
 *   cosine; nothing is renormalised).  An entry depends on its two corpus rows alone -- not on the list positions, on n_cand, on
 *   the other queries of the call or on the wave that computed it -- and G[i][j] and G[j][i] are one value written twice.
 *   Selection, fp32, every product and difference rounded once (no fused multiply-add), oml = 1.0f - lambda:
 *     step 0:     v[d] = lambda * rel[d]
 *     step s > 0: v[d] = (lambda * rel[d]) - (oml * pen[d])
 *     the pick p = the not yet picked, non-padding position with the largest v; ties (-0 == +0 is one) go to the LOWER position;
 *       a candidate whose v is NaN is never picked;
 *     penalty 0 (the maximum over everything picked, the default of the Python surface): pen[d] = G[p][d] after the first pick,
 *       fmaxf(pen[d], G[p][d]) after every later one -- fmaxf keeps a finite pen when G is NaN (a row tombstoned after the scan);
 *     penalty 1 (the last pick only): pen[d] = G[p][d] after every pick.
 *   Outputs, each [n_queries][k] in selection order (1 <= k <= n_cand): out_mmr the v the pick won with, out_rel its rel, out_idx
 *   its entry of cand, out_pos its list position.  When nothing can be picked the remaining outputs are (-inf, -inf, -1, -1).
 *   Workspace (tt_mmr_workspace_bytes, 16-byte aligned): n_queries matrices of Ppad x Ppad floats, Ppad = n_cand rounded up to
 *   16, row-major: G of query q, positions i, j is ((float*)workspace)[(q * Ppad + i) * Ppad + j].  After the call it holds every
 *   entry of non-padding pairs (an entry with a padding position holds +0; nothing is written for n_rows == 0).
 *   Two launches: the Gram tiles (one wave per 16 x 16 block pair on or above the diagonal, operands gathered straight from the
 *   matrix, 16 contiguous bytes of one row per lane and kk), then one workgroup per query whose threads keep lambda * rel, pen
 *   and the taken flags of up to four candidates each in registers and read one row of G per step.
 *   Refused before a launch: dim not a multiple of 128 up to 1024, n_cand outside 1 .. 1024, k outside 1 .. n_cand, penalty not
 *   0 or 1 (TT_E_UNSUPPORTED); lambda NaN or outside [0, 1], n_queries < 0, n_rows < 0, a null array (TT_E_INVALID); a workspace
 *   that is NULL, misaligned or too small (TT_E_WORKSPACE for the size).  n_queries == 0 returns 0 and writes nothing. */
size_t tt_mmr_workspace_bytes(int n_queries, int n_cand);
int tt_mmr_select(const void* corpus_bf16, int64_t n_rows, int dim,
                  const int32_t* cand, const float* rel, int n_queries, int n_cand, int k,
                  float lambda, int penalty, int32_t idx_base,
                  float* out_mmr, float* out_rel, int32_t* out_idx, int32_t* out_pos,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- metadata-filtered exact search ----------------------------------------
 * Replaces the `where=` metadata filter of the reference's vector-store query
 * (src/tensortruth/rag_engine.py:286-365 builds it; index.as_retriever(filters=...)).
 * Every filterable key is dictionary-encoded per row: codes[row] is an int32, 0 = key absent.  The host evaluates each clause once
 * over the key's distinct values into a bitset over codes (bit c set = code c passes; bit 0 is never set), so every operator is
 * the same device test.
 *
 * tt_filter_rows: rows r of [seg_offsets_host[0], seg_offsets_host[n_segments]) (NULL: one segment [0, n_rows)) that pass
 * n_clauses (1..8) clauses, combined with AND (any = 0) or OR (any = 1); clause c is (codes_host[c]: device code column of
 * n_rows entries, bitsets_host[c]: device bitset of ceil(n_codes_host[c] / 32) words; codes >= n_codes do not pass).
 * Writes the passing rows in ASCENDING order to out_rows (capacity: the rows evaluated) and out_offsets[s] (device,
 * n_segments + 1 entries) = list position of segment s's first row; out_offsets[n_segments] = the count.  No atomics: the list
 * is deterministic.  n_segments <= 64.
 *
 * tt_scan_topk_rows: the exact top-k of tt_scan_topk over exactly the rows a tt_filter_rows list names (rows, list_offsets:
 * both read on the device, no host round trip between the two calls).  max_rows = a host-side upper bound on the rows listed
 * per segment (it sizes the workspace and picks the dense or the streaming path; a list longer than it raises status bit 8).
 * Scores and indices are bit-identical to tt_scan_topk over the gathered rows (same fragments, MFMA order and selection),
 * indices mapped back to rows.  seg_offsets_host == NULL: one segment, out [n_queries][k], index = idx_base + row.
 * Otherwise the segments of tt_filter_rows (n_segments + 1 row offsets): out [n_queries][n_segments][k], indices
 * SEGMENT-LOCAL rows (row - seg_offsets_host[s]).  Padding (-inf, -1).  status_flag as in tt_scan_topk (non-zero: re-run
 * tt_scan_topk_exact over the gathered rows). */
size_t tt_filter_rows_workspace_bytes(int64_t n_rows);
int tt_filter_rows(int n_clauses, const int32_t* const* codes_host, const uint32_t* const* bitsets_host,
                   const int32_t* n_codes_host, int any, int64_t n_rows,
                   const int64_t* seg_offsets_host, int n_segments,
                   int32_t* out_rows, int32_t* out_offsets,
                   void* workspace, size_t workspace_bytes, void* stream);
size_t tt_scan_topk_rows_workspace_bytes(int64_t max_rows, int dim, int n_queries, int k);
int tt_scan_topk_rows(const void* corpus_bf16, int64_t n_rows, int dim,
                      const void* queries_bf16, int n_queries, int k,
                      const int32_t* rows, const int32_t* list_offsets, int64_t max_rows,
                      const int64_t* seg_offsets_host, int n_segments, int32_t idx_base,
                      float* out_scores, int32_t* out_idx,
                      void* workspace, size_t workspace_bytes, int32_t* status_flag, void* stream);

/* Merge per-shard partial top-k lists (the step after the RCCL all-gather of
 * SURVEY.md section 8e; also MultiIndexRetriever's concatenate+sort,
 * rag_engine.py:463-507, when indexes live in one matrix).
 * in_scores/in_idx: [n_queries][n_lists * k_in] (per query, lists concatenated);
 * entries with idx < 0 are padding.  Output ordered by (score desc, idx asc).
 * The contract in full (tests/select_refs.py states it in numpy; every scan's final selection follows it too):
 *   an entry is LIVE iff its score is not NaN and its idx is >= 0 -- (finite, idx < 0) never ranks, whatever its score, and
 *   (-inf, idx >= 0) IS live: it ranks after every finite score and before the padding; (+inf, idx >= 0) ranks first;
 *   -0 and +0 are one score (idx decides between them; the zero returned is +0);
 *   the caller's idx column is taken as it is: duplicate (score, idx) pairs are all returned, next to each other;
 *   the output is the first k_out live entries, then (-inf, -1); any n_candidates >= 0, rows of out_* are k_out apart. */
int tt_topk_merge(const float* in_scores, const int32_t* in_idx,
                  int n_queries, int n_candidates, int k_out,
                  float* out_scores, int32_t* out_idx, void* stream);


/* ---- encoder (bi-encoder embedder / cross-encoder reranker) --------------------
 * Replaces the transformer forward the reference reaches through
 *   HuggingFaceEmbedding(...)       src/tensortruth/services/model_manager.py:254-260,
 *                                   src/tensortruth/indexing/builder.py:146-152
 *   SentenceTransformerRerank(...)  src/tensortruth/services/model_manager.py:333-337
 * (upstream: sentence-transformers over transformers XLMRobertaModel / BertModel /
 * XLMRobertaForSequenceClassification).
 *
 * Token layout: sequences are PACKED (no padding tokens are computed): token rows
 * [seq_start[b], seq_start[b] + seq_len[b]) belong to sequence b (any start row, sequences may
 * follow each other without a gap: the attention kernels mask the 8-row token groups two
 * sequences share), and the row count n_rows (>= last start + len) is a multiple of 128 -- or 64 / 192:
 * up to 256 rows (one query, a handful of short texts) the projections run as weight-streaming skinny GEMMs;
 * rows that belong to no sequence are computed but never read.
 * All weights are bf16 [out][in] (nn.Linear layout), biases / LayerNorm parameters fp32.
 * The structs below hold DEVICE pointers but live in HOST memory.
 */
typedef struct tt_layer_weights {
    const void* qkv_w;   /* [3H][H]  query, key, value rows concatenated */
    const float* qkv_b;  /* [3H] */
    const void* o_w;     /* [H][H]   attention.output.dense */
    const float* o_b;
    const float* ln1_g;  /* attention.output.LayerNorm */
    const float* ln1_b;
    const void* ffn1_w;  /* [F][H]   intermediate.dense (GELU-erf) */
    const float* ffn1_b;
    const void* ffn2_w;  /* [H][F]   output.dense */
    const float* ffn2_b;
    const float* ln2_g;  /* output.LayerNorm */
    const float* ln2_b;
    /* Optional fp8 (OCP e4m3) copies of the two projections whose input is a LayerNorm output, with one
     * fp32 scale per output row: w ~= w8 * wscale[out].  When every layer has them (and hidden, ffn and
     * n_rows are multiples of 256) the forward runs those GEMMs on the fp8 matrix cores, quantising the
     * LayerNorm outputs per token; NULL = bf16 (BASELINE.json config 5, "fp8 MFMA reranker"). */
    const void* qkv_w8;      /* [3H][H] bytes */
    const float* qkv_wscale; /* [3H] */
    const void* ffn1_w8;     /* [F][H] bytes */
    const float* ffn1_wscale;/* [F] */
    /* ... and of the other two: the attention output (its input, the attention context, is quantised per
     * token by a row pass) and the FFN output projection, whose input -- the GELU output, rows of F values
     * spread over F/256 tiles -- is written as e4m3 by the FFN-up epilogue with ONE static scale per layer,
     * ffn_act_scale (> 0; from a calibration forward: tt_encoder_weights.ffn_absmax_out). */
    const void* o_w8;        /* [H][H] bytes */
    const float* o_wscale;   /* [H] */
    const void* ffn2_w8;     /* [H][F] bytes */
    const float* ffn2_wscale;/* [H] */
    float ffn_act_scale;     /* 0 = FFN output projection stays bf16 */
} tt_layer_weights;

typedef struct tt_encoder_weights {
    int32_t hidden, layers, heads, ffn, vocab, max_pos, type_vocab;
    float ln_eps;
    const void* word_emb;  /* [vocab][H] bf16 */
    const void* pos_emb;   /* [max_pos][H] bf16 */
    const void* type_emb;  /* [type_vocab][H] bf16 */
    const float* emb_ln_g;
    const float* emb_ln_b;
    const tt_layer_weights* layer; /* host array [layers] */
    const void* cls_dense_w;  /* [H][H] bf16 or NULL (no classification head) */
    const float* cls_dense_b;
    const void* cls_out_w;    /* [1][H] bf16 */
    const float* cls_out_b;   /* [1] */
    /* calibration hook: device float[layers] (zero it first); every forward that produces the bf16 FFN
     * intermediate raises entry l to max |GELU output| of layer l.  NULL = off. */
    float* ffn_absmax_out;
} tt_encoder_weights;

size_t tt_encoder_workspace_bytes(const tt_encoder_weights* w, int n_rows);

/* ids/pos/type_ids: [n_rows] int32 (type_ids may be NULL = all zero: every row reads type row 0); hidden_out:
 * [n_rows][H] bf16 last hidden state.  max_len = longest sequence (host value).
 * An id, a position or a type outside its table is clamped to the nearer end (below 0: row 0; vocab, max_pos or type_vocab and
 * beyond: the last row) -- in every forward of this header (tt_encoder_forward, _f16, _f32, _x3, _f16c and their _cls forms); no
 * row is read outside a table.  With layers = 0 the forward is the embedding sum (word[id] + pos[p]) + type[t] in fp32 and its
 * LayerNorm, written straight to hidden_out. */
int tt_encoder_forward(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                       const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                       int n_seq, int n_rows, int max_len, void* hidden_out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Same forward, but the LAST layer is evaluated for the CLS row of every sequence only (the one row the
 * pooling and the classification head read): cls_out is [round_up(n_seq, 256)][H] bf16 (rows beyond round_up(n_seq, 64)
 * are not written when n_seq <= 256), row b = final hidden state of token seq_start[b].  Identical arithmetic for those rows up to the attention kernel used for the
 * single query row (fp32 probabilities instead of bf16); saves 1/24 of the encoder work at 24 layers. */
size_t tt_encoder_cls_workspace_bytes(const tt_encoder_weights* w, int n_rows, int n_seq);
int tt_encoder_forward_cls(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                           const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                           int n_seq, int n_rows, int max_len, void* cls_out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* sentence-transformers Pooling(cls) + Normalize: out[b] = h[rows[b]] / max(||h[rows[b]]||_2, 1e-12): an all-zero row gives
 * exactly the zero vector.  out_bf16 (optional; NULL: nothing is written) is out_f32 rounded to nearest even in bf16, ready to be
 * a scan query.  Only the n_seq rows of the outputs are written.  hidden % 8 == 0 and <= 1024, else -2; ld >= hidden, ld % 8 == 0,
 * else -1; n_seq = 0 returns 0 and writes nothing.  (The same holds for tt_embed_pool_mean and tt_embed_pool_last.) */
int tt_embed_pool(const void* hidden_bf16, int ld, const int32_t* rows, int n_seq, int hidden,
                  float* out_f32, void* out_bf16, void* stream);

/* sentence-transformers Pooling(mean) + Normalize for checkpoints whose 1_Pooling/config.json says so (e5, all-MiniLM, gte ...;
 * the reference loads any HuggingFace embedding model its config names, services/model_manager.py:188-272):
 * out[b] = mean over the sequence's rows [seq_start[b], seq_start[b] + seq_len[b]) of h, L2-normalised.  hidden: the FULL last
 * hidden state (tt_encoder_forward / _f32 / _x3), bf16 or fp32.  out[b] = m / max(||m||_2, 1e-12) with m the fp32 mean summed in the
 * token order: a mean of exactly zero, and an empty sequence (seq_len[b] <= 0: no row is read), give exactly the zero vector. */
int tt_embed_pool_mean(const void* hidden_bf16, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden,
                       float* out_f32, void* out_bf16, void* stream);
int tt_embed_pool_mean_f32(const float* hidden_f32, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden,
                           float* out_f32, void* out_bf16, void* stream);

/* XLMRobertaClassificationHead + CrossEncoder sigmoid on the CLS rows:
 * scores[b] = sigmoid(out_proj(tanh(dense(h[rows[b]])))) ; logits optional.
 * workspace >= 2 * round_up(round_up(n_seq, 128) * H * 2, 256) bytes: the gathered rows zero-padded to
 * round_up(n_seq, 128), then tanh(dense(.)) of them; nothing behind those bytes is written. */
int tt_rerank_head(const tt_encoder_weights* w, const void* hidden_bf16, const int32_t* rows, int n_seq,
                   float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* Semantic splitter distances (reference: SemanticSplitterNodeParser built at
 * src/tensortruth/indexing/builder.py:393-407): out_dist[i] = 1 - cos(e[i], e[i+1]) for the
 * n consecutive sentence-group embeddings e (fp32 [n][hidden], e.g. tt_embed_pool's output). */
int tt_adjacent_cosine(const float* emb_f32, int n, int hidden, float* out_dist, void* stream);

/* Building blocks, exported for the parity tests (same kernels the forward uses).
 * tt_attention_varlen: Q and K are row-major [rows][ld_qk] at column offsets q_col0 / k_col0;
 * V is passed in the token-blocked transposed layout the QKV GEMM epilogue writes,
 * vt[(row / 8) * ldvt + feature * 8 + row % 8] with ldvt = 8 * heads * head_dim. */
/* tt_gemm_bf16: m, n multiples of 128 and k of 64 (tiled kernels), or m a multiple of 64 up to 256 with n % 16 == 0 and
 * k % 32 == 0 (weight-streaming skinny kernel; same bits as the tiled kernels for the same rows).
 * Non-finite pre-activations (a . w + bias): a NaN gives NaN under every epilogue, in bf16 and in fp16 (tt_gemm_f16 saturates
 * finite values and infinities at +-65504 and keeps a NaN).  The GELU (epilogue 1) of +inf and of -inf is NaN, not +inf and -0:
 * the fitted form computes |x| 2^Q(|x|), i.e. inf * 0; finite inputs of any size are right (GELU(3e38) = 3e38, GELU(-3e38) = 0).
 * tanh (epilogue 3) of +-inf is +-1.  GELU and tanh of -0 give +0 or -0. */
int tt_gemm_bf16(const void* a, const void* w, const float* bias, const void* residual, void* c,
                 int m, int n, int k, int epilogue /*0 bias,1 gelu,2 +residual,3 tanh,7 relu*/, void* stream);
/* tt_layernorm_bf16: hidden % 8 == 0 and <= 1024, else -2; rows = 0 returns 0 and writes nothing; a row of NaN comes out as NaN
 * and changes no other row.  (The same holds for tt_layernorm_f16 and tt_layernorm_bf16_fp8.) */
int tt_layernorm_bf16(const void* in, void* out, const float* gamma, const float* beta, int rows, int hidden,
                      float eps, void* stream);
int tt_attention_varlen(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out,
                        int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads,
                        int head_dim, int max_len, void* stream);
/* tt_attention_cls_varlen: the CLS-only kernel of the last layer on tt_attention_varlen's operands -- the first row of every
 * sequence as the only query; out [n_seq][ld_out] (row b = sequence b).  head_dim 32 or 64; a max_len whose score buffer
 * (max_len + 14 rounded down to 8 floats: up to 7 leading slots of the aligned key frame) exceeds 160 KiB is refused. */
int tt_attention_cls_varlen(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out,
                            int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads,
                            int head_dim, int max_len, void* stream);

/* fp8 building blocks (same kernels the fp8 forward uses).
 * tt_quantize_rows_fp8: q[r][c] = e4m3(x[r][c] * 448 / absmax_r), scale[r] = absmax_r / 448 (1 for a zero row).
 * tt_layernorm_bf16_fp8: tt_layernorm_bf16 that also emits that quantisation of its bf16 output.
 * tt_gemm_fp8: c = epi((a8 . w8^T) * a_scale[m] * w_scale[n] + bias), m, n, k multiples of 256, epilogue 0 / 1. */
int tt_quantize_rows_fp8(const void* in_bf16, int rows, int cols, void* out_fp8, float* out_scale, void* stream);
int tt_layernorm_bf16_fp8(const void* in, void* out, const float* gamma, const float* beta, int rows, int hidden,
                          float eps, void* out_fp8, float* out_scale, void* stream);
int tt_gemm_fp8(const void* a8, const float* a_scale, const void* w8, const float* w_scale, const float* bias, void* c,
                int m, int n, int k, int epilogue /*0 bias, 1 gelu*/, void* stream);
/* ... with the residual epilogue (epilogue 2: + residual[m][n], bf16) or, epilogues 0 / 1, an e4m3 result instead of
 * the bf16 one: c_fp8[m][n] = e4m3(bf16(result) * c_fp8_inv_scale) (c_bf16 is then not written and may be NULL). */
int tt_gemm_fp8_ex(const void* a8, const float* a_scale, const void* w8, const float* w_scale, const float* bias,
                   const void* residual, void* c_bf16, void* c_fp8, float c_fp8_inv_scale, int m, int n, int k,
                   int epilogue, void* stream);

/* ---- reference-precision (fp32) forward -------------------------------------------------------------------
 * The reference's default embedder / reranker dtype is fp32 (src/tensortruth/app_utils/config_schema.py:66-76:
 * torch_dtype None; services/model_manager.py:218-229 passes torch_dtype only when configured).  These entry points
 * run the same encoder with fp32 weights, fp32 activations and fp32 MFMA (v_mfma_f32_32x32x2_f32, exact f32
 * arithmetic at 1/16 of the bf16 matrix rate) for callers that ask for model_kwargs={"torch_dtype": "float32"}:
 * scores within 1e-3 relative of the CPU reference, at interactive batch sizes (one query's candidate pairs).
 * Same packed token layout as tt_encoder_forward; n_rows is any count >= last start + len.
 * All weight tensors fp32, [out][in] for matrices. */
typedef struct tt_layer_weights_f32 {
    const float* qkv_w;  /* [3H][H] */
    const float* qkv_b;
    const float* o_w;    /* [H][H] */
    const float* o_b;
    const float* ln1_g;
    const float* ln1_b;
    const float* ffn1_w; /* [F][H] */
    const float* ffn1_b;
    const float* ffn2_w; /* [H][F] */
    const float* ffn2_b;
    const float* ln2_g;
    const float* ln2_b;
} tt_layer_weights_f32;

typedef struct tt_encoder_weights_f32 {
    int32_t hidden, layers, heads, ffn, vocab, max_pos, type_vocab;
    float ln_eps;
    const float* word_emb;  /* [vocab][H] */
    const float* pos_emb;   /* [max_pos][H] */
    const float* type_emb;  /* [type_vocab][H] */
    const float* emb_ln_g;
    const float* emb_ln_b;
    const tt_layer_weights_f32* layer; /* host array [layers] */
    const float* cls_dense_w;  /* [H][H] or NULL */
    const float* cls_dense_b;
    const float* cls_out_w;    /* [1][H] */
    const float* cls_out_b;    /* [1] */
} tt_encoder_weights_f32;

size_t tt_encoder_f32_workspace_bytes(const tt_encoder_weights_f32* w, int n_rows);
/* hidden_out: [n_rows][H] fp32 last hidden state */
int tt_encoder_forward_f32(const tt_encoder_weights_f32* w, const int32_t* ids, const int32_t* pos,
                           const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                           int n_seq, int n_rows, int max_len, float* hidden_out,
                           void* workspace, size_t workspace_bytes, void* stream);
/* tt_embed_pool / tt_rerank_head on an fp32 hidden state (head workspace >= 2 * round_up(round_up(n_seq, 128) * H * 4, 256) bytes,
 * laid out as tt_rerank_head's; the pooling takes any hidden > 0 and ld >= hidden, and its out_bf16 is bf16 as well) */
int tt_embed_pool_f32(const float* hidden_f32, int ld, const int32_t* rows, int n_seq, int hidden,
                      float* out_f32, void* out_bf16, void* stream);
int tt_rerank_head_f32(const tt_encoder_weights_f32* w, const float* hidden_f32, const int32_t* rows, int n_seq,
                       float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* building block (parity tests): c = epi(a . w^T + bias), fp32; any m, n % 128 == 0, k % 32 == 0;
 * epilogue 0 bias, 1 exact-erf GELU, 2 + residual, 3 tanh */
int tt_gemm_f32(const float* a, const float* w, const float* bias, const float* residual, float* c,
                int m, int n, int k, int epilogue, void* stream);

/* ---- fp16 compute mode (round 3): the same forward with IEEE fp16 activations / weights and v_mfma_*_f16 ---------------------
 * Same weight struct (the matrices then point at fp16 data: word / position / type tables, all projections, the head), same
 * workspace sizes, same argument meaning as the functions they twin; hidden states and V^T are fp16.  Values beyond +-65504
 * saturate at the GEMM / LayerNorm outputs instead of becoming infinite.  No fp8 projections, no split planes in this mode.
 * (FlagEmbedding loads these very models with use_fp16=True by default; the reference's torch_dtype: "float16",
 * app_utils/config_schema.py:66-76, lands here instead of being mapped to bf16.) */
size_t tt_encoder_workspace_bytes_f16(const tt_encoder_weights* w, int n_rows);
size_t tt_encoder_cls_workspace_bytes_f16(const tt_encoder_weights* w, int n_rows, int n_seq);
int tt_encoder_forward_f16(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                           const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                           int n_seq, int n_rows, int max_len, void* hidden_out,
                           void* workspace, size_t workspace_bytes, void* stream);
int tt_encoder_forward_cls_f16(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                               const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                               int n_seq, int n_rows, int max_len, void* cls_out,
                               void* workspace, size_t workspace_bytes, void* stream);
/* The pooling of an fp16 hidden state: tt_embed_pool's / tt_embed_pool_mean's contract, except that the optional 16-bit output is
 * out_f32 rounded to nearest even in IEEE fp16 (NOT bf16: a scan query is rounded to bf16 from out_f32 by the caller).  The head's
 * workspace is tt_rerank_head's (2-byte elements). */
int tt_embed_pool_f16(const void* hidden_f16, int ld, const int32_t* rows, int n_seq, int hidden, float* out_f32,
                      void* out_f16, void* stream);
int tt_embed_pool_mean_f16(const void* hidden_f16, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden,
                           float* out_f32, void* out_f16, void* stream);
int tt_rerank_head_f16(const tt_encoder_weights* w, const void* hidden_f16, const int32_t* rows, int n_seq,
                       float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* building blocks (parity tests) */
int tt_gemm_f16(const void* a, const void* w, const float* bias, const void* residual, void* c,
                int m, int n, int k, int epilogue, void* stream);
int tt_layernorm_f16(const void* in, void* out, const float* gamma, const float* beta, int rows, int hidden,
                     float eps, void* stream);
int tt_attention_varlen_f16(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out,
                            int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads,
                            int head_dim, int max_len, void* stream);
int tt_attention_cls_varlen_f16(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out,
                                int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads,
                                int head_dim, int max_len, void* stream);

/* ---- reference precision on the bf16 matrix cores: split-bf16 ("bf16x3") forward -------------------------------------
 * Same contract as the fp32 forward above (the unchanged reference call SentenceTransformerRerank(model=, top_n=, device=),
 * src/tensortruth/services/model_manager.py:333-337, and HuggingFaceEmbedding with torch_dtype None,
 * app_utils/config_schema.py:66-76, are fp32), at a third of the bf16 path's rate instead of a sixteenth: every matrix
 * product runs on v_mfma_*_bf16 with both operands split into two bf16 planes (x = hi + lo, hi = bf16(x),
 * lo = bf16(x - hi); a.b ~= a_hi.b_hi + a_hi.b_lo + a_lo.b_hi, fp32 accumulate), the residual stream, LayerNorm, softmax
 * and the exact-erf GELU stay fp32.  Scores within 1e-3 relative of the CPU reference (measured ~1e-5).
 * "Planes" = bf16 [rows][2 W]: columns [0, W) hold hi, [W, 2 W) hold lo.  Weight matrices are planes [out][2 in];
 * embedding tables, biases, LayerNorm parameters and the classification head are fp32.  hidden a multiple of 256 (<= 1024)
 * with head_dim 64, ffn a multiple of 256, n_rows a multiple of 256. */
typedef struct tt_layer_weights_x3 {
    const void* qkv_w;   /* planes [3H][2H] */
    const float* qkv_b;
    const void* o_w;     /* planes [H][2H] */
    const float* o_b;
    const float* ln1_g;
    const float* ln1_b;
    const void* ffn1_w;  /* planes [F][2H] */
    const float* ffn1_b;
    const void* ffn2_w;  /* planes [H][2F] */
    const float* ffn2_b;
    const float* ln2_g;
    const float* ln2_b;
} tt_layer_weights_x3;

typedef struct tt_encoder_weights_x3 {
    int32_t hidden, layers, heads, ffn, vocab, max_pos, type_vocab;
    float ln_eps;
    const float* word_emb;  /* [vocab][H] fp32 */
    const float* pos_emb;
    const float* type_emb;
    const float* emb_ln_g;
    const float* emb_ln_b;
    const tt_layer_weights_x3* layer; /* host array [layers] */
    const float* cls_dense_w;  /* [H][H] fp32 or NULL */
    const float* cls_dense_b;
    const float* cls_out_w;
    const float* cls_out_b;
} tt_encoder_weights_x3;

size_t tt_encoder_x3_workspace_bytes(const tt_encoder_weights_x3* w, int n_rows);
/* hidden_out: [n_rows][H] fp32 last hidden state (pool it with tt_embed_pool_f32) */
int tt_encoder_forward_x3(const tt_encoder_weights_x3* w, const int32_t* ids, const int32_t* pos,
                          const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                          int n_seq, int n_rows, int max_len, float* hidden_out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* classification head on the fp32 hidden state (workspace as tt_rerank_head_f32) */
/* Same forward with the LAST layer evaluated for the first row (CLS) of every sequence only -- the split-bf16 twin of
 * tt_encoder_forward_cls: cls_out [pad(n_seq)][hidden] fp32, pad = n_seq rounded up to 64 (<= 256 sequences) or to 256. */
size_t tt_encoder_x3_cls_workspace_bytes(const tt_encoder_weights_x3* w, int n_rows, int n_seq);
int tt_encoder_forward_x3_cls(const tt_encoder_weights_x3* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                              const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                              float* cls_out, void* workspace, size_t workspace_bytes, void* stream);
/* the head of the fp32-residual paths runs on the fp32 kernels: tt_rerank_head_f32 on these fp32 head weights, bit for bit, with
 * its workspace (also tt_rerank_head_x3_f16 and tt_rerank_head_f16c) */
int tt_rerank_head_x3(const tt_encoder_weights_x3* w, const float* hidden_f32, const int32_t* rows, int n_seq,
                      float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* building blocks (parity tests).  tt_split_planes: fp32 [rows][cols] -> planes [rows][2 cols], cols % 4 == 0.
 * tt_gemm_x3: a planes [m][2k], w planes [n][2k]; m, n multiples of 256, k of 64; epilogue 0 bias / 1 exact-erf GELU ->
 * c_planes [m][2n]; epilogue 2 -> c_f32 [m][n] = a.w^T + bias + residual_f32 [m][n].
 * tt_attention_x3: Q / K planes in one buffer (hi at q_col0 / k_col0 + head * 64, lo lo_off columns further), V in the
 * token-blocked transposed layout of tt_attention_varlen, once per plane; context planes out (hi at head * 64, lo at
 * out_lo_off + head * 64). */
int tt_split_planes(const float* in_f32, int64_t rows, int cols, void* out_planes, void* stream);
int tt_gemm_x3(const void* a_planes, const void* w_planes, const float* bias, const float* residual_f32, void* c_planes,
               float* c_f32, int m, int n, int k, int epilogue, void* stream);
/* tt_gemm_x3_ex: a test building block, as tt_gemm_fp8_ex is -- tt_gemm_x3 with the layouts and epilogues the forward itself
 * uses.  Epilogues 0 / 1 write c_planes [m][ldc], hi at column 0 and lo at column c_lo_off (c_lo_off >= n, ldc >= c_lo_off + n;
 * the forward's Q | K projection: ldc = 4 H, c_lo_off = 2 H); epilogue 2 writes c_f32 [m][ldc] = a.w^T + bias + residual, the
 * residual EITHER as residual_f32 [m][ldr] OR as residual_planes [m][ldr] (hi at column 0, lo at column res_lo_off: hi + lo is
 * rebuilt in fp32 -- the forward on fp16 planes: ldr = 2 H, res_lo_off = H); epilogue 5 (V^T) writes the V8 layout of
 * tt_attention_varlen twice, vt_hi and vt_lo [m / 8][ldvt >= 8 n], element (m, n) at (m / 8) * ldvt + 8 n + m % 8.  Arguments
 * an epilogue does not use may be NULL / 0.  Shapes as tt_gemm_x3: up to 256 rows m % 64 == 0, n % 16 == 0, k % 32 == 0;
 * beyond that m % 256 == 0, n % 64 == 0, k % 64 == 0, k >= 128; leading dimensions and offsets keep 16-byte alignment.
 * Non-finite pre-activations (tests/test_gemm_x3_edges_gpu.py): a NaN stays a NaN in both planes.  Epilogue 0 (and 5: the same
 * packing) splits +-inf as the host does: bf16 planes hi = +-inf, lo = NaN; fp16 planes hi = lo = +-65504 (both saturate: finite values up to +-131008 are
 * carried as 65504 + the rest).  The GELU of +inf is that split of +inf; of -inf, NaN in both planes (inf * 0). */
int tt_gemm_x3_ex(const void* a_planes, const void* w_planes, const float* bias, const float* residual_f32,
                  const void* residual_planes, int ldr, int res_lo_off, void* c_planes, int ldc, int c_lo_off, float* c_f32,
                  void* vt_hi, void* vt_lo, int ldvt, int m, int n, int k, int epilogue, void* stream);
int tt_attention_x3(const void* qk_planes, int ld_qk, int q_col0, int k_col0, int lo_off, const void* vt_hi,
                    const void* vt_lo, int ldvt, void* out_planes, int ld_out, int out_lo_off,
                    const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads, int max_len, void* stream);
/* tt_attention_x3_hd: tt_attention_x3 with head_dim 32 or 64 (scale 1 / sqrt(head_dim)); cls_only = 1 runs the CLS-only
 * kernel of the last layer instead -- out_planes then holds one row per sequence (row b = sequence b's first query), and a
 * max_len past its score buffer (as tt_attention_cls_varlen) is refused. */
int tt_attention_x3_hd(const void* qk_planes, int ld_qk, int q_col0, int k_col0, int lo_off, const void* vt_hi,
                       const void* vt_lo, int ldvt, void* out_planes, int ld_out, int out_lo_off,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads, int max_len,
                       int head_dim, int cls_only, void* stream);

/* ---- reference precision on TWO matrix-time units: the "f16c" forward (csrc/f16c_path.hip, round 4) --------------------
 * What the reference's unchanged calls compute -- fp32 semantics (services/model_manager.py:333-337 passes no dtype;
 * app_utils/config_schema.py:66-76: torch_dtype None) -- at half the bf16 matrix rate instead of split-bf16's third: every
 * GEMM operand is carried as "c-planes", hi = fp16(x) plus two OCP e4m3 planes (x and x - hi) with one E8M0 block exponent
 * per 32 elements, and a product runs as  hi.hi (fp16 MFMA) + e4m3(a).e4m3(w_lo) + e4m3(a_lo).e4m3(w)  (block-scaled MFMA at
 * twice the rate; the cross terms are 2^-12 of the result).  Attention on single fp16 products, fp32 softmax; residual
 * stream, LayerNorm, exact-erf GELU and the head in fp32.  Scores within 1e-3 relative of the CPU path (measured 1e-4).
 * Weights: matrices as c-planes in the weight flavour [out][hi: 2 in | lo8: in | x8: in] bytes + tiled scales, both made by
 * tt_f16c_quantize(weight = 1) from the fp32 tensor; tables, biases, LayerNorm parameters and the head fp32.
 * hidden a multiple of 256 (<= 1024) with head_dim 64, ffn a multiple of 256, n_rows a multiple of 256. */
typedef struct tt_layer_weights_f16c {
    const void* qkv_w;   /* c-planes [3H][4H bytes] */
    const void* qkv_s;   /* tiled scales, tt_f16c_scale_bytes(3H, H, 1) bytes */
    const float* qkv_b;
    const void* o_w;     /* [H][4H bytes] */
    const void* o_s;
    const float* o_b;
    const float* ln1_g;
    const float* ln1_b;
    const void* ffn1_w;  /* [F][4H bytes] */
    const void* ffn1_s;
    const float* ffn1_b;
    const void* ffn2_w;  /* [H][4F bytes] */
    const void* ffn2_s;
    const float* ffn2_b;
    const float* ln2_g;
    const float* ln2_b;
} tt_layer_weights_f16c;

typedef struct tt_encoder_weights_f16c {
    int32_t hidden, layers, heads, ffn, vocab, max_pos, type_vocab;
    float ln_eps;
    const float* word_emb;  /* [vocab][H] fp32 */
    const float* pos_emb;
    const float* type_emb;
    const float* emb_ln_g;
    const float* emb_ln_b;
    const tt_layer_weights_f16c* layer; /* host array [layers] */
    const float* cls_dense_w;  /* [H][H] fp32 or NULL */
    const float* cls_dense_b;
    const float* cls_out_w;
    const float* cls_out_b;
} tt_encoder_weights_f16c;

size_t tt_encoder_f16c_workspace_bytes(const tt_encoder_weights_f16c* w, int n_rows);
/* hidden_out: [n_rows][H] fp32 last hidden state (pool it with tt_embed_pool_f32 / tt_embed_pool_mean_f32) */
int tt_encoder_forward_f16c(const tt_encoder_weights_f16c* w, const int32_t* ids, const int32_t* pos,
                            const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                            int n_seq, int n_rows, int max_len, float* hidden_out,
                            void* workspace, size_t workspace_bytes, void* stream);
/* the LAST layer for the first row (CLS) of every sequence only: cls_out [pad(n_seq)][hidden] fp32, pad = n_seq rounded up to 256 */
size_t tt_encoder_f16c_cls_workspace_bytes(const tt_encoder_weights_f16c* w, int n_rows, int n_seq);
int tt_encoder_forward_f16c_cls(const tt_encoder_weights_f16c* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                                const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                                float* cls_out, void* workspace, size_t workspace_bytes, void* stream);
int tt_rerank_head_f16c(const tt_encoder_weights_f16c* w, const float* hidden_f32, const int32_t* rows, int n_seq,
                        float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* building blocks (weight preparation, parity tests).
 * tt_f16c_quantize: fp32 [rows][k] (k a multiple of 256) -> c-planes [rows][4 k bytes] + tiled scales
 *   (tt_f16c_scale_bytes(rows, k, weight) bytes); weight = 0: activation flavour [hi | x8 | lo8], 1: weight flavour
 *   [hi | lo8 | x8] with two scale parts.  Rows are padded to 256 in the scale array only.
 * tt_gemm_f16c: a c-planes [m][4k], w c-planes [n][4k]; m, n, k multiples of 256; epilogue 0: fp16 c_out [m][n] =
 *   a.w^T + bias; 1: exact-erf GELU -> c-planes c_out [m][4n] + c_scales; 2: fp32 c_out [m][n] = a.w^T + bias + residual_f32.
 * tt_attention_f16c: Q / K as two fp16 planes in one buffer (hi at q_col0 / k_col0 + head * 64, lo lo_off columns further:
 *   the score product runs on three fp16 products), V fp16 in the V8 layout of tt_attention_varlen, head_dim 64; context as c-planes. */
size_t tt_f16c_scale_bytes(int64_t rows, int k, int weight);
int tt_f16c_quantize(const float* in_f32, int64_t rows, int k, int weight, void* out_planes, void* out_scales, void* stream);
int tt_gemm_f16c(const void* a_planes, const void* a_scales, const void* w_planes, const void* w_scales, const float* bias,
                 const float* residual_f32, void* c_out, void* c_scales, int m, int n, int k, int epilogue, void* stream);
int tt_attention_f16c(const void* qk_f16, int ld_qk, int q_col0, int k_col0, int lo_off, const void* vt_f16, int ldvt, void* out_planes,
                      void* out_scales, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads, int max_len,
                      void* stream);

/* ---- "f16x3": the split-plane forward above with fp16 planes (csrc/x3_path.hip compiled a second time, round 4) -------
 * Same entry points, same layouts, `_f16` suffix: a value is carried as hi = fp16(x), lo = fp16(x - hi) -- 22 significand
 * bits per operand instead of the two bf16 planes' 16, down to fp16's subnormal grid: |x - hi - lo| <= max(2^-22 |x|, 2^-25)
 * inside +-65504 (the lo plane is an fp16 subnormal for every |x| < 2^-3) -- and a product as three v_mfma_*_f16 products.  It is the DEFAULT
 * implementation of the reference precision: on weights with trained-model statistics (attention logits of ~100, scores
 * down to 0.005: tests/stress_weights.py) it holds 1e-3 relative with a margin where bf16x3 sits AT the bar and the
 * two-unit f16c path is 7x outside.  Values beyond +-65504 saturate in the hi plane (the lo plane takes what is left). */
size_t tt_encoder_x3_workspace_bytes_f16(const tt_encoder_weights_x3* w, int n_rows);
int tt_encoder_forward_x3_f16(const tt_encoder_weights_x3* w, const int32_t* ids, const int32_t* pos,
                              const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len,
                              int n_seq, int n_rows, int max_len, float* hidden_out,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t tt_encoder_x3_cls_workspace_bytes_f16(const tt_encoder_weights_x3* w, int n_rows, int n_seq);
int tt_encoder_forward_x3_cls_f16(const tt_encoder_weights_x3* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                                  const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                                  float* cls_out, void* workspace, size_t workspace_bytes, void* stream);
int tt_rerank_head_x3_f16(const tt_encoder_weights_x3* w, const float* hidden_f32, const int32_t* rows, int n_seq,
                          float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream);
int tt_split_planes_f16(const float* in_f32, int64_t rows, int cols, void* out_planes, void* stream);
int tt_gemm_x3_f16(const void* a_planes, const void* w_planes, const float* bias, const float* residual_f32, void* c_planes,
                   float* c_f32, int m, int n, int k, int epilogue, void* stream);
int tt_gemm_x3_ex_f16(const void* a_planes, const void* w_planes, const float* bias, const float* residual_f32,
                      const void* residual_planes, int ldr, int res_lo_off, void* c_planes, int ldc, int c_lo_off, float* c_f32,
                      void* vt_hi, void* vt_lo, int ldvt, int m, int n, int k, int epilogue, void* stream);
int tt_attention_x3_f16(const void* qk_planes, int ld_qk, int q_col0, int k_col0, int lo_off, const void* vt_hi,
                        const void* vt_lo, int ldvt, void* out_planes, int ld_out, int out_lo_off,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads, int max_len, void* stream);
int tt_attention_x3_hd_f16(const void* qk_planes, int ld_qk, int q_col0, int k_col0, int lo_off, const void* vt_hi,
                           const void* vt_lo, int ldvt, void* out_planes, int ld_out, int out_lo_off,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads, int max_len,
                           int head_dim, int cls_only, void* stream);

/* ---- decoder embedder / reranker: Qwen3Model-architecture checkpoints (Qwen3-Embedding, Qwen3ForSequenceClassification;
 * csrc/decoder.hip) ------------------------------------------------------------------------------------------------------
 * The reference embeds with whatever Hugging Face model its config names (api/routes/startup.py:108-133,
 * app_utils/config_schema.py:41-61, services/model_manager.py:214-252); the Qwen3-Embedding model card runs it in bf16 with
 * left padding and pools the LAST token.  Pre-norm decoder block, no biases: RMSNorm -> QKV projection -> per-head RMSNorm of
 * q and k, rotate-half RoPE (positions 0-based within each sequence) -> causal grouped-query attention (query head h reads KV
 * head h / (heads / kv_heads)) -> output projection + residual -> RMSNorm -> gate|up projection -> SiLU(gate) * up -> down
 * projection + residual; a final RMSNorm.  Same packed token layout as tt_encoder_forward (`pos` = position within the
 * sequence, type_ids must be NULL), same projections (the 16-bit GEMMs), bf16 -- or fp16 for the `_f16` twins.
 * Matrices [out][in] in the element type, norm weights fp32.  hidden a multiple of 128 and <= 1024 (the scan's limit),
 * head_dim 64 or 128, heads a multiple of kv_heads, (heads + 2 kv_heads) * head_dim a multiple of 128, heads * head_dim and
 * ffn multiples of 64; anything else is refused before a launch. */
typedef struct tt_decoder_layer_weights {
    const void* qkv_w;        /* [(heads + 2 kv_heads) * head_dim][H]: q_proj, k_proj, v_proj rows concatenated */
    const float* q_norm;      /* [head_dim] self_attn.q_norm */
    const float* k_norm;      /* [head_dim] self_attn.k_norm */
    const void* o_w;          /* [H][heads * head_dim] */
    const float* attn_norm;   /* [H] input_layernorm */
    const float* ffn_norm;    /* [H] post_attention_layernorm */
    const void* gate_up_w;    /* [2F][H]: gate_proj rows, then up_proj rows */
    const void* down_w;       /* [H][F] */
} tt_decoder_layer_weights;

typedef struct tt_decoder_weights {
    int32_t hidden, layers, heads, kv_heads, head_dim, ffn, vocab;
    float rms_eps, rope_theta;
    const void* embed;        /* [vocab][H] embed_tokens */
    const tt_decoder_layer_weights* layer; /* host array [layers] */
    const float* final_norm;  /* [H] norm */
} tt_decoder_weights;

size_t tt_decoder_workspace_bytes(const tt_decoder_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state (after the final norm) */
int tt_decoder_forward(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The pooled-row tail (rerankers, last-token embedders): the same forward, of which only ONE row per sequence is wanted.
 * pool_row: device [n_seq], the absolute row of the token to keep, seq_start[b] <= pool_row[b] < seq_start[b] + seq_len[b] (a row
 * outside its sequence gives a zero context for that sequence, never an access outside the batch).  Layers 0 .. layers-2 run as in
 * tt_decoder_forward.  In the last layer Q, K and V are produced for every row (a pooled query attends to all keys before it), but
 * attention, output projection + residual, the MLP and the final norm run for the n_seq pooled rows only, on compact buffers of
 * P rows, P = n_seq rounded up to 64 (n_seq <= 256) or to 256.  hidden_out: [P][H]; row b < n_seq holds the bits row pool_row[b]
 * of tt_decoder_forward's output holds (the projections give a row the same bits whatever else is in the batch; the attention
 * evaluates the 16-query tile of pool_row[b] exactly as the full kernel does and stores that one query); rows n_seq .. P-1 are
 * zero.  layers == 0: embedding -> final norm of the pooled rows.  Same workspace as the full forward (the compact buffers reuse it). */
size_t tt_decoder_rows_workspace_bytes(const tt_decoder_weights* w, int n_rows, int n_seq);   /* 0 for a refused shape */
int tt_decoder_forward_rows(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                            const int32_t* pool_row, void* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
/* Score head of Qwen3ForSequenceClassification (one label, Linear(H, 1, bias=False)): logits[b] = hidden[b] . score_w in fp32,
 * scores[b] = sigmoid(logits[b]); hidden [n_seq][ld] in the element type (the tail's output), score_w fp32 [H], both 16-byte
 * aligned; logits optional. */
int tt_decoder_score(const void* hidden, int ld, const float* score_w, int n_seq, int hidden_size, float* scores, float* logits,
                     void* stream);
/* sentence-transformers Pooling(lasttoken) + Normalize: out[b] = h[r] / max(||h[r]||_2, 1e-12) with r = seq_start[b] + seq_len[b] - 1;
 * an all-zero row gives exactly the zero vector, and so does an empty sequence (seq_len[b] <= 0), of which no row is read.
 * out_16 (optional) is out_f32 rounded to nearest even in the element type (bf16: ready to be a scan query; IEEE fp16 from
 * tt_embed_pool_last_f16).  hidden_size % 8 == 0 and <= 1024, else -2; ld >= hidden_size, ld % 8 == 0, else -1. */
int tt_embed_pool_last(const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden_size,
                       float* out_f32, void* out_16, void* stream);
/* building blocks (parity tests; the forward's own kernels).
 * tt_qk_norm_rope: rows of qkv [n_rows][ld] (q heads at column h * head_dim, k heads behind them, v heads behind those; n_rows a
 *   multiple of 8): q and k heads RMSNorm-ed with q_norm / k_norm and rotated by RoPE at pos[row] in place; the v heads copied to
 *   the V8 layout of tt_attention_varlen, vt[(row / 8) * ldvt + feature * 8 + row % 8].
 * tt_attention_causal_gqa: out[q][h * head_dim ...] = softmax over keys seq_start <= k <= q of (Q_h . K_{h/g}) / sqrt(head_dim),
 *   applied to V_{h/g}; Q at q_col0 + h * head_dim, K at k_col0 + kvh * head_dim of rows of ld elements, V in the V8 layout; any
 *   sequence start; rows of no sequence are not written. */
int tt_qk_norm_rope(void* qkv, int ld, const int32_t* pos, const float* q_norm, const float* k_norm, int n_rows, int heads,
                    int kv_heads, int head_dim, float eps, float rope_theta, void* vt, int ldvt, void* stream);
int tt_attention_causal_gqa(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads,
                            int head_dim, int max_len, void* stream);
/* the fp16 twins (decoder.hip compiled a second time, like the encoder's _f16 entry points) */
size_t tt_decoder_workspace_bytes_f16(const tt_decoder_weights* w, int n_rows);
int tt_decoder_forward_f16(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t tt_decoder_rows_workspace_bytes_f16(const tt_decoder_weights* w, int n_rows, int n_seq);
int tt_decoder_forward_rows_f16(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                                const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                                const int32_t* pool_row, void* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
int tt_decoder_score_f16(const void* hidden, int ld, const float* score_w, int n_seq, int hidden_size, float* scores, float* logits,
                         void* stream);
int tt_embed_pool_last_f16(const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden_size,
                           float* out_f32, void* out_16, void* stream);
int tt_qk_norm_rope_f16(void* qkv, int ld, const int32_t* pos, const float* q_norm, const float* k_norm, int n_rows, int heads,
                        int kv_heads, int head_dim, float eps, float rope_theta, void* vt, int ldvt, void* stream);
int tt_attention_causal_gqa_f16(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                                const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads,
                                int head_dim, int max_len, void* stream);

/* ---- ModernBERT encoders: embedders and ModernBertForSequenceClassification cross-encoders (csrc/modernbert.hip) -----------
 * gte-modernbert, gte-reranker-modernbert, nomic modernbert-embed and the answerdotai/ModernBERT fine-tunes.  Pre-norm encoder
 * block without biases: h = LayerNorm(tok_embeddings[ids]) (weight only; no position table, no token types); per layer
 *   x = attn_norm(h) (layer 0: none) -> Wqkv -> rotate-half RoPE of q and k with the layer's base (positions 0-based within each
 *   sequence) -> bidirectional attention over the sequence's own tokens, on a "sliding" layer restricted to keys with
 *   |q - k| <= local_attention / 2 -> Wo + residual -> mlp_norm -> Wi ([2F][H]: "input" rows, then "gate" rows) ->
 *   GELU_erf(input) * gate -> mlp.Wo + residual;
 * a final LayerNorm.  Same packed token layout as tt_encoder_forward (`pos` = position within the sequence, type_ids must be
 * NULL), same projections (the 16-bit GEMMs), bf16 -- or fp16 for the `_f16` twins.  Matrices [out][in] in the element type, norm
 * weights fp32.  hidden a multiple of 128 and <= 1024, hidden = 64 * heads (head_dim 64), ffn a multiple of 64; anything else is
 * refused before a launch. */
typedef struct tt_modernbert_layer_weights {
    const void* qkv_w;        /* [3H][H] attn.Wqkv: q rows, k rows, v rows */
    const void* o_w;          /* [H][H] attn.Wo */
    const float* attn_norm;   /* [H], NULL for a layer without one (layer 0) */
    const float* mlp_norm;    /* [H] */
    const void* wi_w;         /* [2F][H] mlp.Wi */
    const void* wo_w;         /* [H][F] mlp.Wo */
    int32_t sliding;          /* 1: a sliding_attention layer (window, local RoPE base); 0: full_attention (global base) */
} tt_modernbert_layer_weights;

typedef struct tt_modernbert_weights {
    int32_t hidden, layers, heads, ffn, vocab, local_attention;
    float norm_eps, global_rope_theta, local_rope_theta;
    const void* embed;        /* [vocab][H] embeddings.tok_embeddings */
    const float* emb_norm;    /* [H] embeddings.norm */
    const tt_modernbert_layer_weights* layer; /* host array [layers] */
    const float* final_norm;  /* [H] */
    /* classification head (tt_modernbert_head; NULL for an embedder), all fp32 */
    const float* head_dense_wt; /* [H][H] head.dense.weight TRANSPOSED: [in][out] */
    const float* head_norm;     /* [H] head.norm */
    const float* cls_w;         /* [H] classifier.weight (one label) */
    const float* cls_b;         /* [1] classifier.bias */
} tt_modernbert_weights;

size_t tt_modernbert_workspace_bytes(const tt_modernbert_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state (after the final norm) */
int tt_modernbert_forward(const tt_modernbert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                          const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Head of ModernBertForSequenceClassification, one label, fp32 arithmetic: p = hidden[seq_start[b]] (pooling 0, "cls") or the mean
 * of the sequence's rows (pooling 1, "mean"); logits[b] = classifier(LayerNorm(GELU_erf(head.dense(p)))), scores[b] =
 * sigmoid(logits[b]); hidden [.][ld] in the element type (tt_modernbert_forward's output); logits optional. */
int tt_modernbert_head(const tt_modernbert_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                       int n_seq, int pooling, float* scores, float* logits, void* stream);
/* building blocks (parity tests; the forward's own kernels).
 * tt_rope_v8: rows of qkv [n_rows][ld] (q heads at column h * 64, k heads behind them, v heads behind those; n_rows a multiple of
 *   8): q and k heads rotated by rotate-half RoPE of base rope_theta at pos[row] in place (angles in fp32); the v heads copied to
 *   the V8 layout of tt_attention_varlen, vt[(row / 8) * ldvt + feature * 8 + row % 8].
 * tt_attention_window: out[q][h * 64 ...] = softmax over the keys k of q's own sequence with |q - k| <= window of
 *   (Q_h . K_h) / 8, applied to V_h (window < 0: every key of the sequence); Q at q_col0 + h * 64, K at k_col0 + h * 64 of rows of
 *   ld elements, V in the V8 layout; any sequence start; rows of no sequence are not written.  head_dim must be 64. */
int tt_rope_v8(void* qkv, int ld, const int32_t* pos, int n_rows, int heads, int head_dim, float rope_theta, void* vt, int ldvt,
               void* stream);
int tt_attention_window(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                        int max_len, int window, void* stream);
/* the fp16 twins (modernbert.hip compiled a second time) */
size_t tt_modernbert_workspace_bytes_f16(const tt_modernbert_weights* w, int n_rows);
int tt_modernbert_forward_f16(const tt_modernbert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                              const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                              void* workspace, size_t workspace_bytes, void* stream);
int tt_modernbert_head_f16(const tt_modernbert_weights* w, const void* hidden, int ld, const int32_t* seq_start,
                           const int32_t* seq_len, int n_seq, int pooling, float* scores, float* logits, void* stream);
int tt_rope_v8_f16(void* qkv, int ld, const int32_t* pos, int n_rows, int heads, int head_dim, float rope_theta, void* vt, int ldvt,
                   void* stream);
int tt_attention_window_f16(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                            int max_len, int window, void* stream);

/* ---- EmbeddingGemma embedders: Gemma3TextModel with use_bidirectional_attention (google/embeddinggemma-300m; csrc/gemma.hip) ----
 * With norm(v; w) = v * rsqrt(mean(v^2) + eps) * (1 + w) (note the 1 + w): h = embed_tokens[ids] * embed_scale (no position
 * table, no token types); per layer, four norms around two sublayers, the residual added AFTER the post-norm:
 *   x = norm(h; input_norm) -> q | k | v projection -> per-head norm of q and k (q_norm, k_norm), rotate-half RoPE with the layer
 *   type's base (positions 0-based within each sequence) -> bidirectional grouped-query attention over the sequence's own tokens
 *   (query head h reads KV head h / (heads / kv_heads); scale 1 / sqrt(head_dim)), on a "sliding" layer restricted to keys with
 *   |q - k| <= window -> o projection -> h = h + norm(.; post_attn_norm) -> x = norm(h; pre_ffn_norm) -> gate | up projection ->
 *   GELU_tanh(gate) * up -> down projection -> h = h + norm(.; post_ffn_norm);
 * a final norm.  `window` is what the kernels compare with: transformers rewrites a bidirectional config's sliding_window S to
 * S / 2 + 1 when it loads it and masks with |q - k| < that value, so a config.json holding S means window = S / 2.
 * Same packed token layout as tt_encoder_forward (`pos` = position within the sequence, type_ids must be NULL), same projections
 * (the 16-bit GEMMs), bf16 only: the model card rules fp16 out, and there are no `_f16` twins.  Matrices [out][in] in bf16, norm
 * weights fp32 as the checkpoint stores them (w, not 1 + w).  hidden a multiple of 128 and <= 1024 (the scan's limit), head_dim 256,
 * heads a multiple of kv_heads, (heads + 2 kv_heads) * head_dim a multiple of 128, heads * head_dim and ffn multiples of 64; anything
 * else is refused before a launch. */
typedef struct tt_gemma_layer_weights {
    const void* qkv_w;           /* [(heads + 2 kv_heads) * head_dim][H]: q_proj, k_proj, v_proj rows concatenated */
    const float* q_norm;         /* [head_dim] self_attn.q_norm */
    const float* k_norm;         /* [head_dim] self_attn.k_norm */
    const void* o_w;             /* [H][heads * head_dim] */
    const float* input_norm;     /* [H] input_layernorm */
    const float* post_attn_norm; /* [H] post_attention_layernorm */
    const float* pre_ffn_norm;   /* [H] pre_feedforward_layernorm */
    const float* post_ffn_norm;  /* [H] post_feedforward_layernorm */
    const void* gate_up_w;       /* [2F][H]: gate_proj rows, then up_proj rows */
    const void* down_w;          /* [H][F] */
    int32_t sliding;             /* 1: a sliding_attention layer (window, local RoPE base); 0: full_attention (global base) */
} tt_gemma_layer_weights;

typedef struct tt_gemma_weights {
    int32_t hidden, layers, heads, kv_heads, head_dim, ffn, vocab, window;
    float rms_eps, global_rope_theta, local_rope_theta;
    float embed_scale;           /* sqrt(hidden) rounded to bf16, as Gemma3TextScaledWordEmbedding rounds it to the weights' type */
    const void* embed;           /* [vocab][H] embed_tokens */
    const tt_gemma_layer_weights* layer; /* host array [layers] */
    const float* final_norm;     /* [H] norm */
    /* the sentence-transformers Dense modules behind the pooling (tt_gemma_pool_dense), fp32, no bias, identity activation */
    int32_t dense1_out, dense2_out;
    const float* dense1_wt;      /* [H][dense1_out]: 2_Dense linear.weight TRANSPOSED ([in][out]) */
    const float* dense2_wt;      /* [dense1_out][dense2_out]: 3_Dense linear.weight TRANSPOSED */
} tt_gemma_weights;

size_t tt_gemma_workspace_bytes(const tt_gemma_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state (after the final norm) */
int tt_gemma_forward(const tt_gemma_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                     const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* sentence-transformers Pooling(mean) -> Dense -> Dense -> Normalize in fp32: p = the mean of the sequence's rows of hidden
 * [.][ld] bf16 (tt_gemma_forward's output), summed in ascending order; v = dense2(dense1(p)); out_f32[b] = v / max(||v||, 1e-12),
 * [n_seq][dense2_out]; out_16 (optional) the same vector in bf16 (ready to be a scan query).  dense1_out a multiple of 64 up to
 * 3072, dense2_out a multiple of 64 up to 1024.  A workgroup handles eight sequences, so the matrices are read once per eight; a
 * sequence's vector does not depend on the batch it travels in. */
int tt_gemma_pool_dense(const tt_gemma_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                        int n_seq, float* out_f32, void* out_16, void* stream);
/* building blocks (parity tests; the forward's own kernels), bf16, head_dim 256.
 * tt_gemma_qk_norm_rope: tt_qk_norm_rope's arguments and layout; q and k heads normalised with (1 + q_norm) / (1 + k_norm) and
 *   rotated at pos[row] with base rope_theta in place, the v heads copied to the V8 layout.
 * tt_gemma_add_norm: rows of H elements; h_out = h + norm(y; norm_a), x_out = norm(h + norm(y; norm_a); norm_b), both from the
 *   unrounded sum and rounded once.  y NULL: x_out = norm(h; norm_b) only (norm_a, h_out unused).  The four buffers are distinct.
 * tt_attention_window_gqa: out[q][h * head_dim ...] = softmax over the keys k of q's own sequence with |q - k| <= window of
 *   (Q_h . K_{h/g}) / sqrt(head_dim), applied to V_{h/g} (window < 0: every key of the sequence); Q at q_col0 + h * head_dim, K at
 *   k_col0 + kvh * head_dim of rows of ld elements, V in the V8 layout; any sequence start; rows of no sequence are not written. */
int tt_gemma_qk_norm_rope(void* qkv, int ld, const int32_t* pos, const float* q_norm, const float* k_norm, int n_rows, int heads,
                          int kv_heads, int head_dim, float eps, float rope_theta, void* vt, int ldvt, void* stream);
int tt_gemma_add_norm(const void* y, const void* h, const float* norm_a, const float* norm_b, int n_rows, int hidden, float eps,
                      void* h_out, void* x_out, void* stream);
int tt_attention_window_gqa(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads,
                            int head_dim, int max_len, int window, void* stream);

/* ---- MPNet encoders: MPNetModel embedders (csrc/mpnet.hip) ---------------------------------------------------------------------
 * sentence-transformers/all-mpnet-base-v2, all-mpnet-base-v1, multi-qa-mpnet-base-dot-v1 / -cos-v1.  The post-LN block of
 * tt_encoder_forward (separate q / k / v / o projections with biases, concatenated to the [3H][H] layout; exact-erf GELU) with two
 * differences: the embeddings are LayerNorm(word[id] + position[pos]) -- no token types; positions start at padding_idx + 1 = 2,
 * as in XLM-R -- and every layer's attention adds a learned relative-position bias to the scores before the softmax,
 *   softmax(q . k / 8 + rel_bias[bucket(key - query)][h]),  bidirectional within the sequence,
 * one [32 buckets][heads] table for all layers; bucket = MPNetEncoder.relative_position_bucket with 32 buckets and max_distance
 * 128 (both hard-coded in transformers): with n = query - key, 16 [n < 0] + f(|n|), f(m) = m below 8, else
 * min(15, 8 + trunc(log(m / 8) / log(16) * 8)).  Every distance beyond +-128 falls into the last bucket of its side, so the bias
 * of a distance is ONE lookup in a per-head table over the clamped distance, which the caller builds when it loads the weights:
 *   bias_table[h][d + 128] = rel_bias[bucket(d)][h] * log2(e),  d = key - query in [-128, 128]      ([heads][257] fp32).
 * Same packed token layout as tt_encoder_forward (type_ids must be NULL), the same projections and LayerNorms, bf16 -- or fp16 for
 * the `_f16` twins.  enc.type_emb, the classification head and ffn_absmax_out are not read.  hidden a multiple of 128 and <= 1024,
 * hidden = 64 * heads (head_dim 64), ffn a multiple of 128, no fp8 pointer in any layer; anything else is refused before a
 * launch. */
typedef struct tt_mpnet_weights {
    tt_encoder_weights enc;   /* the encoder's tensors (type_emb, cls_*, ffn_absmax_out unused) */
    const float* rel_bias;    /* [32][heads] fp32: attention.relative_attention_bias.weight as the checkpoint stores it -- what
                                 bias_table was built from; must be present, the kernels read bias_table */
    const float* bias_table;  /* [heads][257] fp32, see above */
} tt_mpnet_weights;

size_t tt_mpnet_workspace_bytes(const tt_mpnet_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state */
int tt_mpnet_forward(const tt_mpnet_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                     const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* building block (parity tests; the forward's own kernel): tt_attention_window's operands without a window, plus the bias --
 *   out[q][h * 64 ...] = softmax over the keys k of q's own sequence of (Q_h . K_h) / 8 + bias_table[h][clamp(k - q, -128, 128) + 128]
 *   / log2(e), applied to V_h.  An all-zero table gives tt_attention_window's bits (window < 0).  head_dim must be 64. */
int tt_attention_relbias(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                         const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                         int max_len, const float* bias_table, void* stream);
/* the fp16 twins (mpnet.hip compiled a second time) */
size_t tt_mpnet_workspace_bytes_f16(const tt_mpnet_weights* w, int n_rows);
int tt_mpnet_forward_f16(const tt_mpnet_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                         const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                         void* workspace, size_t workspace_bytes, void* stream);
int tt_attention_relbias_f16(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                             const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                             int max_len, const float* bias_table, void* stream);

/* ---- DeBERTa-v2 / v3 cross-encoders: DebertaV2ForSequenceClassification (csrc/deberta.hip) ------------------------------------
 * mixedbread-ai/mxbai-rerank-xsmall-v1 / -base-v1 / -large-v1, the deberta-v3 checkpoints under cross-encoder/, fine-tunes of
 * microsoft/deberta-v3-{xsmall,small,base,large}.  The post-LN block of tt_encoder_forward (separate query / key / value / output
 * projections with biases, concatenated to the [3H][H] layout; exact-erf GELU) with two differences: the embeddings are
 * LayerNorm(word[id]) -- no absolute positions (position_biased_input false), no token types -- and every layer's attention is
 * DISENTANGLED (pos_att_type c2p + p2c, share_att_key): for query q and key k of a sequence and head h, 64 wide,
 *   i(q, k) = clamp(bucket(q - k) + span, 0, 2 span - 1),  span = position_buckets, bucket = make_log_bucket_position
 *   score   = (Q[q] . K[k] + Q[q] . PK[i(q, k)] + K[k] . PQ[i(q, k)]) / sqrt(3 * 64),  softmax over the sequence's keys,
 * PK / PQ = this layer's key / query projection (with bias) of LayerNorm(encoder.rel_embeddings)[0 : 2 span].  Both depend on the
 * weights only: the caller computes them when it loads the checkpoint (pos_key / pos_query, [n_pos][H] in the element type,
 * n_pos = 2 span), and the index as a table over the distance, so that no logarithm runs on the device:
 *   dist_index[d + max_pos - 1] = i for d = q - k in [-(max_pos - 1), max_pos - 1]       (int32 [2 max_pos - 1], non-decreasing).
 * Per layer one launch writes the two position score tables into the workspace in fp32,
 *   C[t][h][w] = Q[t,h] . PK[w,h],  P[t][h][w] = K[t,h] . PQ[w,h]   (w over the indices the batch's max_len reaches),
 * and the attention adds C[q][h][i] + P[k][h][i] to the raw score of every live pair: n_rows * heads * n_pos * 8 bytes of
 * workspace beside the encoder's buffers.
 * Same packed token layout as tt_encoder_forward; type_ids must be NULL; pos must be present and its values are not used.  bf16, or
 * fp16 for the `_f16` twins.  enc.pos_emb, enc.type_emb, enc.cls_* and ffn_absmax_out are not read.  hidden a multiple of 128 and
 * <= 1024, hidden = 64 * heads (head_dim 64), ffn a multiple of 128, n_pos a positive multiple of 4, max_pos <= 512, max_len <=
 * max_pos, no fp8 pointer in any layer, tables that fit in size_t; anything else is refused before a launch. */
typedef struct tt_deberta_weights {
    tt_encoder_weights enc;        /* the encoder's tensors (pos_emb, type_emb, cls_*, ffn_absmax_out unused; enc.max_pos unused) */
    const void* const* pos_key;    /* host array [layers]: layer l's PK, device [n_pos][H] in the element type, 16-byte aligned */
    const void* const* pos_query;  /* host array [layers]: layer l's PQ, likewise */
    const int32_t* dist_index;     /* device [2 max_pos - 1], see above; entries are clamped to [0, n_pos - 1] when read */
    int32_t n_pos;                 /* 2 * position_buckets */
    int32_t max_pos;               /* max_position_embeddings: the longest sequence */
    /* classification head (tt_deberta_head; NULL for weights without one), all fp32 */
    const float* pooler_dense_wt;  /* [H][H] pooler.dense.weight TRANSPOSED: [in][out] */
    const float* pooler_dense_b;   /* [H] */
    const float* cls_w;            /* [H] classifier.weight (one label) */
    const float* cls_b;            /* [1] classifier.bias */
} tt_deberta_weights;

size_t tt_deberta_workspace_bytes(const tt_deberta_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state */
int tt_deberta_forward(const tt_deberta_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Head of DebertaV2ForSequenceClassification, one label, fp32 arithmetic, tt_modernbert_head's arguments: p = hidden[seq_start[b]]
 * (pooling must be 0; seq_len is not read); logits[b] = classifier(GELU_erf(pooler.dense(p))), scores[b] = sigmoid(logits[b]);
 * hidden [.][ld] in the element type (tt_deberta_forward's output); logits optional. */
int tt_deberta_head(const tt_deberta_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                    int n_seq, int pooling, float* scores, float* logits, void* stream);
/* building block (parity tests; the forward's own kernels): tt_attention_window's operands without a window, plus the position
 * terms -- out[q][h * 64 ...] = softmax over the keys k of q's own sequence of (Q_h[q] . K_h[k] + Q_h[q] . PK_h[i] + K_h[k] . PQ_h[i])
 * / sqrt(192), i = dist_index[q - k + max_pos - 1], applied to V_h.  pos_key / pos_query [n_pos][heads * 64] in the element type;
 * workspace: 2 * align256(n_rows * heads * n_pos * 4) bytes, 256-byte aligned.  head_dim must be 64. */
int tt_attention_disentangled(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                              const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                              int max_len, const void* pos_key, const void* pos_query, int n_pos, const int32_t* dist_index,
                              int max_pos, void* workspace, size_t workspace_bytes, void* stream);
/* the fp16 twins (deberta.hip compiled a second time) */
size_t tt_deberta_workspace_bytes_f16(const tt_deberta_weights* w, int n_rows);
int tt_deberta_forward_f16(const tt_deberta_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                           void* workspace, size_t workspace_bytes, void* stream);
int tt_deberta_head_f16(const tt_deberta_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                        int n_seq, int pooling, float* scores, float* logits, void* stream);
int tt_attention_disentangled_f16(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                                  const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                                  int max_len, const void* pos_key, const void* pos_query, int n_pos, const int32_t* dist_index,
                                  int max_pos, void* workspace, size_t workspace_bytes, void* stream);

/* ---- RoPE-BERT encoders: post-LN BERT blocks with rotary positions (csrc/ropebert.hip) ------------------------------------------
 * NomicBertModel (nomic-ai/nomic-embed-text-v1 / -v1.5) and JinaEmbeddingsV3Model (jina-embeddings-v3 in its transformers format),
 * one layer class in transformers.  No position table; q and k rotated by rotate-half RoPE with one base for every layer
 * (positions 0-based within each sequence, angles in fp32); bidirectional attention over the sequence's own tokens:
 *   h = LayerNorm(word[ids] + type[0]; emb_ln);  per layer
 *   q | k | v = h Wqkv^T (+ b_qkv) -> RoPE(q), RoPE(k) -> a = softmax(q k^T / 8) v -> h = LayerNorm(h + a Wo^T (+ b_o); ln1)
 *   mlp_kind 1 (SwiGLU, NomicBERT): m = (SiLU(h Wgate^T) * (h Wup^T)) Wdown^T                    -- no biases
 *   mlp_kind 0 (GELU, Jina):        m = GELU_erf(h W1^T + b1) W2^T + b2
 *   h = LayerNorm(h + m; ln2);  no final norm.
 * Same packed token layout as tt_encoder_forward (`pos` = position within the sequence; type_ids must be NULL: every token of an
 * embedder call is of type 0, whose row is still added), the same projections (the 16-bit GEMMs) and LayerNorms, tt_rope_v8 and
 * the attention kernel of tt_attention_varlen at every length; bf16 -- or fp16 for the `_f16` twins.  Matrices [out][in] in the
 * element type, norms and biases fp32; a NULL bias pointer means no bias.  hidden a multiple of 128 and <= 1024, hidden = 64 *
 * heads (head_dim 64), ffn a multiple of 64 (of 128 with mlp_kind 0, whose up-projection is ffn columns wide), mlp_kind 0 or 1;
 * anything else is refused before a launch. */
typedef struct tt_ropebert_layer_weights {
    const void* qkv_w;        /* [3H][H]: q_proj, k_proj, v_proj rows concatenated */
    const float* qkv_b;       /* [3H] or NULL */
    const void* o_w;          /* [H][H] self_attn.o_proj */
    const float* o_b;         /* [H] or NULL */
    const float* ln1_g;       /* [H] post_attention_layernorm */
    const float* ln1_b;
    const void* up_w;         /* mlp_kind 1: [2F][H], gate_proj rows then up_proj rows; mlp_kind 0: [F][H] mlp.fc1 */
    const float* up_b;        /* mlp_kind 0: [F] or NULL; mlp_kind 1: NULL */
    const void* down_w;       /* [H][F] down_proj / mlp.fc2 */
    const float* down_b;      /* mlp_kind 0: [H] or NULL; mlp_kind 1: NULL */
    const float* ln2_g;       /* [H] post_mlp_layernorm */
    const float* ln2_b;
} tt_ropebert_layer_weights;

typedef struct tt_ropebert_weights {
    int32_t hidden, layers, heads, ffn, vocab, type_vocab;
    int32_t mlp_kind;         /* 0: GELU_erf(fc1) fc2 with biases; 1: SwiGLU without */
    float ln_eps, rope_theta;
    const void* word_emb;     /* [vocab][H] */
    const void* type_emb;     /* [type_vocab][H]; row 0 is added to every token */
    const float* emb_ln_g;    /* [H] embeddings.LayerNorm */
    const float* emb_ln_b;
    const tt_ropebert_layer_weights* layer; /* host array [layers] */
} tt_ropebert_weights;

size_t tt_ropebert_workspace_bytes(const tt_ropebert_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state */
int tt_ropebert_forward(const tt_ropebert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* the fp16 twins (ropebert.hip compiled a second time) */
size_t tt_ropebert_workspace_bytes_f16(const tt_ropebert_weights* w, int n_rows);
int tt_ropebert_forward_f16(const tt_ropebert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- JinaBERT encoders: post-LN BERT blocks with ALiBi attention and a GEGLU feed-forward (csrc/jinabert.hip) ------------------
 * The remote-code architecture (jinaai/jina-bert-implementation) behind jinaai/jina-embeddings-v2-small-en / -base-en; its
 * config.json says model_type "bert" with position_embedding_type "alibi".  No position table and no RoPE; every head h adds the
 * ALiBi bias -slope_h |query - key| to its scores AFTER the 1 / sqrt(64) scaling, symmetric, bidirectional over the sequence's
 * own tokens; slope_h follows the original ALiBi rule for `heads` heads (a geometric series for a power of two, else the series of
 * the power of two below plus every other term of the next one's):
 *   h = LayerNorm(word[ids] + type[0]; emb_ln);  per layer
 *   q | k | v = h Wqkv^T + b_qkv -> a = softmax(q k^T / 8 - slope_h |i - j|) v -> h = LayerNorm(h + a Wo^T + b_o; ln1)
 *   g = h Wgate^T  [T][2F], no bias -> m = (GELU_erf(g[:, :F]) * g[:, F:]) Wdown^T + b_down -> h = LayerNorm(h + m; ln2)
 * no final norm.  alibi_slope_log2[h] = slope_h * log2(e), computed in double and rounded once by the caller: the kernel works in
 * the log2 domain, x = s * (log2(e) / 8) - alibi_slope_log2[h] * float(|key - query|), in registers -- no table and no clamp, exact
 * at any distance a packed batch can hold.  Same packed token layout as tt_ropebert_forward (`pos` must be present and its values
 * are not used; type_ids must be NULL: every token of an embedder call is of type 0, whose row is still added), the same
 * projections (the 16-bit GEMMs; the QKV epilogue writes V in the V8 layout) and LayerNorms, the gated-activation row op of the
 * ModernBERT path; the attention is tt_attention_alibi at every length.  bf16 -- or fp16 for the `_f16` twins.  Matrices
 * [out][in] in the element type, norms and biases fp32.  hidden a multiple of 128 and <= 1024, hidden = 64 * heads (head_dim 64),
 * ffn a multiple of 128; anything else is refused before a launch with the field named. */
typedef struct tt_jinabert_layer_weights {
    const void* qkv_w;        /* [3H][H]: attention.self.query, .key, .value rows concatenated */
    const float* qkv_b;       /* [3H] */
    const void* o_w;          /* [H][H] attention.output.dense */
    const float* o_b;         /* [H] */
    const float* ln1_g;       /* [H] attention.output.LayerNorm */
    const float* ln1_b;
    const void* gate_w;       /* [2F][H] mlp.gated_layers: the rows GELU is applied to, then the rows that multiply them; no bias */
    const void* down_w;       /* [H][F] mlp.wo */
    const float* down_b;      /* [H] */
    const float* ln2_g;       /* [H] mlp.layernorm */
    const float* ln2_b;
} tt_jinabert_layer_weights;

typedef struct tt_jinabert_weights {
    int32_t hidden, layers, heads, ffn, vocab, type_vocab;
    float ln_eps;
    const void* word_emb;     /* [vocab][H] */
    const void* type_emb;     /* [type_vocab][H]; row 0 is added to every token */
    const float* emb_ln_g;    /* [H] embeddings.LayerNorm */
    const float* emb_ln_b;
    const float* alibi_slope_log2;   /* [heads] fp32, DEVICE memory: slope_h * log2(e) */
    const tt_jinabert_layer_weights* layer; /* host array [layers] */
} tt_jinabert_weights;

size_t tt_jinabert_workspace_bytes(const tt_jinabert_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][H] last hidden state */
int tt_jinabert_forward(const tt_jinabert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* building block (parity tests; the forward's own kernel): tt_attention_window's operands without a window, plus the slopes --
 *   out[q][h * 64 ...] = softmax over the keys k of q's own sequence of (Q_h . K_h) / 8 - slope_log2[h] / log2(e) * |k - q|,
 *   applied to V_h; slope_log2 [heads] fp32 in device memory.  One wave per (16-query tile, sequence, head); rows of no sequence
 *   are not written.  All-zero slopes give attention without a bias.  head_dim must be 64. */
int tt_attention_alibi(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim, int max_len,
                       const float* slope_log2, void* stream);
/* the fp16 twins (jinabert.hip compiled a second time) */
size_t tt_jinabert_workspace_bytes_f16(const tt_jinabert_weights* w, int n_rows);
int tt_jinabert_forward_f16(const tt_jinabert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                            void* workspace, size_t workspace_bytes, void* stream);
int tt_attention_alibi_f16(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                           int max_len, const float* slope_log2, void* stream);

/* ---- T5 encoders: T5EncoderModel embedders (csrc/t5.hip) ------------------------------------------------------------------------
 * sentence-transformers/sentence-t5-base / -large, gtr-t5-base / -large, hkunlp/instructor-base / -large (model_type "t5",
 * transformers/models/t5/modeling_t5.py).  Pre-norm blocks without biases; norm(v; w) = bf16(v * rsqrt(mean(v^2) + eps)) * w
 * (T5LayerNorm: no mean subtraction, fp32 statistics, rounded to the element type BEFORE the weight multiplies):
 *   h = embed[ids]                                           no scaling, no LayerNorm, no position table, no token types
 *   x = norm(h; ln_attn) -> q | k | v = x Wqkv^T -> a = softmax(q . k + rel_bias[bucket(key - query)][head]) v -> h = h + a Wo^T
 *   x = norm(h; ln_ffn)  -> mlp_kind 0 (feed_forward_proj "relu"):        h = h + relu(x wi^T) wo^T
 *                           mlp_kind 1 ("gated-gelu", T5 v1.1 / flan):    h = h + (gelu_new(x wi_0^T) * (x wi_1^T)) wo^T
 *   hidden_out = norm(h; final_norm)
 * T5 does NOT divide the scores by sqrt(d_kv).  The attention is tt_attention_relbias, which computes q . k / 8 + table: THE Q
 * ROWS OF qkv_w (its first d_model rows) ARE STORED PRE-SCALED BY 8 -- a shift of the exponent, exact in bf16, and x (8 W)^T =
 * 8 (x W^T) bit for bit.  The bias table [32 buckets][heads] belongs to block 0 and is added in every block; the bucket function
 * (32 buckets, max_distance 128, bidirectional, key - query) is MPNet's, so bias_table is built the same way:
 *   bias_table[h][d + 128] = rel_bias[bucket(d)][h] * log2(e),  d = key - query in [-128, 128]      ([heads][257] fp32).
 * The ReLU sits in the up-projection's GEMM epilogue (tt_gemm_bf16 epilogue 7): no extra pass over [T][d_ff].
 * Same packed token layout as tt_encoder_forward; `pos` must be present and its values are not used; type_ids must be NULL.
 * Sequences up to 512 tokens, as for MPNet.  bf16 only: the FFN activations leave fp16's range (transformers' fp16 run clamps
 * them, which is another model), so there are no `_f16` twins.  Matrices [out][in] in bf16, norm weights fp32.
 * d_model a multiple of 128 and <= 1024, d_kv = 64 and heads * 64 = d_model, d_ff a multiple of 128, num_buckets = 32,
 * max_distance = 128, mlp_kind 0 or 1, dense_out (with dense_wt) a multiple of 128 and <= 1024; anything else is refused before a
 * launch with the field named. */
typedef struct tt_t5_layer_weights {
    const float* ln_attn;     /* [d_model] layer.0.layer_norm */
    const void* qkv_w;        /* [3 d_model][d_model]: q rows TIMES 8, then k rows, then v rows */
    const void* o_w;          /* [d_model][d_model] SelfAttention.o */
    const float* ln_ffn;      /* [d_model] layer.1.layer_norm */
    const void* wi;           /* mlp_kind 0: [d_ff][d_model] DenseReluDense.wi; mlp_kind 1: [2 d_ff][d_model], wi_0 rows then wi_1 rows */
    const void* wo;           /* [d_model][d_ff] DenseReluDense.wo */
} tt_t5_layer_weights;

typedef struct tt_t5_weights {
    int32_t d_model, layers, heads, d_kv, d_ff, vocab;
    int32_t mlp_kind;         /* 0: relu; 1: gated-gelu (gelu_new) */
    int32_t num_buckets;      /* relative_attention_num_buckets: 32 */
    int32_t max_distance;     /* relative_attention_max_distance: 128 */
    float eps;                /* layer_norm_epsilon */
    const void* embed;        /* [vocab][d_model] shared */
    const tt_t5_layer_weights* layer; /* host array [layers] */
    const float* final_norm;  /* [d_model] encoder.final_layer_norm */
    const float* rel_bias;    /* [32][heads] fp32: block 0's relative_attention_bias.weight as the checkpoint stores it -- what
                                 bias_table was built from; must be present, the kernels read bias_table */
    const float* bias_table;  /* [heads][257] fp32, see above */
    /* the sentence-transformers Dense module behind the pooling (tt_t5_pool_dense), fp32, no bias, identity activation */
    int32_t dense_out;        /* 0 with dense_wt NULL: the checkpoint has no Dense module */
    const float* dense_wt;    /* [d_model][dense_out]: 2_Dense linear.weight TRANSPOSED ([in][out]); NULL: none */
} tt_t5_weights;

size_t tt_t5_workspace_bytes(const tt_t5_weights* w, int n_rows);   /* 0 for a refused shape */
/* hidden_out: [n_rows][d_model] last hidden state (after the final norm) */
int tt_t5_forward(const tt_t5_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                  const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                  void* workspace, size_t workspace_bytes, void* stream);
/* sentence-transformers Pooling(mean) -> Dense (if any) -> Normalize in fp32: p = the mean of the rows seq_start[b] ..
 * seq_start[b] + seq_len[b] - 1 of hidden [.][ld] bf16 (tt_t5_forward's output), summed in ascending order -- any sub-range of a
 * sequence (INSTRUCTOR's include_prompt false: the rows behind the instruction), any row alignment; v = p dense^T, or p itself
 * without a Dense module; out_f32[b] = v / max(||v||, 1e-12), [n_seq][dense_out or d_model]; out_16 (optional) the same vector in
 * bf16 (ready to be a scan query).  A workgroup handles eight sequences, so the matrix is read once per eight; a sequence's vector
 * does not depend on the batch it travels in. */
int tt_t5_pool_dense(const tt_t5_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                     int n_seq, float* out_f32, void* out_16, void* stream);

/* ---- ColBERT late interaction: MaxSim, the per-token projection, key-limited attention (csrc/colbert.hip) -----------------------
 * colbert-ir/colbertv2.0, answerdotai/answerai-colbert-small-v1 and the same models in PyLate's layout: a BERT encoder
 * (tt_encoder_weights) whose every kept token row is projected to `dim` values and L2-normalised.  Passages are encoded once, when
 * they are indexed; at query time only the query runs through the encoder and every candidate is scored over vectors that already
 * sit in device memory.  All pointers are device memory unless said otherwise; 16-bit operands are bf16 -- or fp16 for the `_f16`
 * twins.
 *
 * tt_maxsim: scores[q][c] = sum over i < q_len[q] of max over j < d_len[doc] of <Q[q_start[q] + i], D[d_start[doc] + j]>, doc =
 *   cand[q * n_cand + c] (cand NULL: doc = c for every query).  Vectors are row-major with a row stride of dim.  Products on
 *   mfma_f32_16x16x32 with fp32 accumulation; the maximum starts from -inf; the sum over the query's tokens runs in index order in
 *   fp32, so a score does not depend on which other pairs are in the launch.  A negative candidate writes -inf; a document of
 *   length 0 scores 0.  dim a multiple of 32 up to 128 (anything else is refused before a launch); q_len 1 .. 128, d_len 0 .. 512:
 *   the kernel clamps a length into its range, and the host wrapper (colbert.py), which holds the lengths, refuses one outside it.
 * tt_maxsim_scan_topk: the exact MaxSim top-k over documents 0 .. n_docs-1 for n_q (1 .. 64) queries, k 1 .. 1024, in ONE read of the
 *   store per pass of queries.  Every score is tt_maxsim's value with cand NULL for the same (query, document), bit for bit: one
 *   mfma_f32_16x16x32 chain per <Q_i, D_j> over kk = 0 .. dim/32 - 1 from 0 (document rows the A operand, query rows the B operand),
 *   rows past d_len masked to -inf, the maximum from -inf, the q_len maxima added in index order in fp32 -- so a score does not
 *   depend on n_q, on the other queries of the call, on where the document sits in the store, or on the wave that scored it.  A
 *   document of length 0 scores 0 and is a valid result.  alive: uint8 [n_docs], 0 = a tombstone (NULL: every document is live); a
 *   tombstone is not read, and its slot of the workspace (tt_maxsim_scan_workspace_bytes: n_q rows of n_docs rounded up to 32
 *   floats, which hold every score after the call) holds NaN, which the selection never returns.  Selection: tt_lexical_scan_topk's
 *   (tt_scan_topk_exact's).  out_scores / out_idx [n_q][k], ordered by (score descending, document number ascending), padded with
 *   (-inf, -1); n_docs == 0 writes the padding without a scoring launch.  A persistent grid (two workgroups per compute unit) of
 *   four-wave workgroups; a wave owns whole documents, two consecutive numbers per step of a static grid-stride walk.  The queries'
 *   B fragments are staged in LDS, at most 16 blocks of 16 query rows (256 padded rows: 64 KB at dim 128) at a time: queries that
 *   do not fit are taken in further sweeps of the store inside the same launch (eight 32-token queries, or two 128-token ones, per
 *   sweep).  Refused before a launch: dim not a multiple of 32 up to 128, n_q outside 1 .. 64, k outside 1 .. 1024
 *   (TT_E_UNSUPPORTED); n_docs outside 0 .. INT_MAX, a null output, a null array with n_docs > 0 (TT_E_INVALID); a workspace that is
 *   NULL or too small (TT_E_WORKSPACE).  q_len 1 .. 128 and d_len 0 .. 512 are clamped in the kernel as tt_maxsim clamps them; the
 *   host wrapper (colbert.py) refuses a value outside.
 * tt_colbert_project: for n < n_out, y = W hidden[rows[n]] (W [dim][H], no bias, fp32 accumulation), out[n] = y / max(||y||_2, 1e-12)
 *   in fp32, rounded once; out [n_out][dim].  Nothing is computed for rows that are not listed; a row number outside [0, n_rows)
 *   and an all-zero row give zeros.  H a multiple of 128 up to 1024, dim as above.
 * tt_attention_keylimit: tt_attention_varlen's operands plus key_len [n_seq]: every one of a sequence's seq_len rows is a query,
 *   only its first key_len[b] rows are keys (clamped into [1, seq_len]; the host wrapper refuses a value outside).  Sequences of up
 *   to 128 rows, at any start row (a neighbour's rows in a shared 8-row group are masked); head_dim 32 or 64.  Rows of no
 *   sequence are not written.
 * tt_encoder_forward_keylen: tt_encoder_forward with that attention in every layer (same workspace: tt_encoder_workspace_bytes);
 *   max_len <= 128. */
int tt_maxsim(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs, const int64_t* d_start,
              const int32_t* d_len, const int32_t* cand, int n_cand, int dim, float* scores, void* stream);
size_t tt_maxsim_scan_workspace_bytes(int64_t n_docs, int n_q);   /* one size for both element types */
int tt_maxsim_scan_topk(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs,
                        const int64_t* d_start, const int32_t* d_len, const uint8_t* alive, int64_t n_docs, int dim, int k,
                        float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);
int tt_colbert_project(const void* hidden, int n_rows, int H, const void* w, int dim, const int32_t* rows, int n_out, void* out,
                       void* stream);
int tt_attention_keylimit(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                          const int32_t* seq_start, const int32_t* seq_len, const int32_t* key_len, int n_seq, int heads, int head_dim,
                          int max_len, void* stream);
int tt_encoder_forward_keylen(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                              const int32_t* seq_start, const int32_t* seq_len, const int32_t* key_len, int n_seq, int n_rows,
                              int max_len, void* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
/* the fp16 twins (colbert.hip and encoder_api.hip compiled a second time) */
int tt_maxsim_f16(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs, const int64_t* d_start,
                  const int32_t* d_len, const int32_t* cand, int n_cand, int dim, float* scores, void* stream);
int tt_maxsim_scan_topk_f16(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs,
                            const int64_t* d_start, const int32_t* d_len, const uint8_t* alive, int64_t n_docs, int dim, int k,
                            float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);
int tt_colbert_project_f16(const void* hidden, int n_rows, int H, const void* w, int dim, const int32_t* rows, int n_out, void* out,
                           void* stream);
int tt_attention_keylimit_f16(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                              const int32_t* seq_start, const int32_t* seq_len, const int32_t* key_len, int n_seq, int heads,
                              int head_dim, int max_len, void* stream);
int tt_encoder_forward_keylen_f16(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                                  const int32_t* seq_start, const int32_t* seq_len, const int32_t* key_len, int n_seq, int n_rows,
                                  int max_len, void* hidden_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Lexical weights and hybrid scoring: BGE-M3's sparse head (csrc/lexical.hip) -----------------------------------------------
 * BAAI/bge-m3 ships a second head, sparse_linear.pt (weight [1][H], bias [1]): the forward pass that gives the dense vector also
 * gives a weight per token, t_i = relu(<w, h_i> + b) over the last hidden state.  A text's lexical vector holds, for every
 * distinct token id it contains except four ids that are left out (<s>, </s>, <pad>, <unk>), the maximum of t_i over the id's
 * occurrences, where that is > 0; lex(q, d) = sum over the ids both hold of q_w * d_w.  Passages are encoded once, when they are
 * indexed, into CSR arrays in device memory; a query costs one short forward and a scoring kernel.  All pointers are device
 * memory unless named _host.
 *
 * tt_lexical_weights: hidden [n_rows][ld] (ld >= H, even; row stride in elements) and w [H] are bf16 -- fp16 for the `_f16` twin,
 *   fp32 for `_f32` (the reference-precision paths' hidden states); ids int32 [n_rows]: the token id of every row; seq_start,
 *   seq_len int32 [n_seq] (tt_encoder_forward's arrays).  For sequence b, with s = seq_start[b]:
 *     out_nnz[b]                     the number of distinct kept ids: ids other than skip0..3_host (a value that is no id, e.g. -1,
 *                                    leaves nothing out) and not negative, whose maximum weight is > 0
 *     out_terms[s .. s+out_nnz[b])   those ids in ascending order
 *     out_weights[s .. s+out_nnz[b]) their weights, max over the id's rows of <w, hidden[row]> + bias_host
 *     slots s+out_nnz[b] .. s+seq_len[b]-1 hold term -1 and weight 0.
 *   Rows of no sequence are not written (out_terms [n_rows] int32, out_weights [n_rows] fp32; out_weights also carries the
 *   pre-activations between the entry point's two launches).  The dot product is accumulated in fp32 -- products of the operands
 *   converted to fp32, fmaf -- in an order that depends on H alone (lane l of a wave takes elements 128 c + 2 l and + 1 for
 *   ascending c, then a butterfly over the 64 lanes), and the bias is added last: a sequence's output is the same bits alone or in
 *   any batch, at any start row.  The maximum is exact (a sort of (id, weight) pairs in LDS).  H a multiple of 128 up to 1024,
 *   max_len (>= every seq_len) 1 .. 8192, n_seq up to 65535: anything else is refused before a launch.  The sort's LDS image is
 *   sized by max_len (64, 512, 2048 or 8192 pairs of 8 bytes); a seq_len beyond that class is clamped to it, a sequence is cut at
 *   n_rows, and one with a negative start writes out_nnz 0 only.
 * tt_lexical_score: for query q and candidate c, doc = cand[q * n_cand + c] (cand NULL: doc = c for every query),
 *     out_lex[q][c]    = sum over ids in both entries of q_w * d_w
 *     out_dense[q][c]  = <q_dense[q], d_dense[doc]>
 *     out_hybrid[q][c] = (w_dense * out_dense + w_lex * out_lex) / (w_dense + w_lex)
 *   all fp32 [n_q][n_cand].  Query q's entry is q_terms / q_weights [q_start[q] .. + q_nnz[q]), document doc's entry d_terms /
 *   d_weights [d_start[doc] .. + d_nnz[doc]); terms int32, weights fp32, ASCENDING and distinct by term within an entry -- a
 *   precondition (the output of tt_lexical_weights has it).  q_dense [n_q][dim], d_dense [n_docs][dim] bf16, indexed by document
 *   number.  q_dense NULL: lexical only, out_dense and out_hybrid are not written (and dim, w_dense, w_lex not read).  One wave
 *   per pair: lane l adds the products of the document's entries l, l + 64, ... that the query holds, in that order, in fp32
 *   (fmaf), then a butterfly over the lanes; the dense part likewise over dim (bf16 operands converted to fp32, fmaf, lane l
 *   elements 128 c + 2 l and + 1).  A pair scores the same bits wherever it sits in cand, with or without cand, in any batch.  A
 *   negative candidate and a document with d_nnz < 0 (a tombstone) write -inf to every output that is written; d_nnz == 0 or no
 *   shared id gives lex = 0.  dim a multiple of 128 up to 1024, w_dense, w_lex >= 0 and not both 0 (refused before a launch
 *   otherwise).  q_nnz 0 .. 512, d_nnz -1 .. 8192: the kernel clamps a length into its range, and the host wrapper (lexical.py),
 *   which holds the lengths, refuses one outside it.  Document numbers in cand must be < the number of documents (the wrapper
 *   checks).
 * tt_lexical_scan_topk: the exact lexical top-k over documents 0 .. n_docs-1 for n_q (1 .. 64) queries, k 1 .. 1024.  Scores are
 *   tt_lexical_score's bits with cand NULL, written to the workspace (tt_lexical_scan_workspace_bytes: n_q rows of n_docs rounded
 *   up to 32 floats); a tombstone's slot holds NaN there, which the selection never returns (what a deleted row of the dense
 *   index scores).  Selection: tt_scan_topk_exact's.  out_scores / out_idx [n_q][k], ordered by (score descending, document
 *   number ascending), padded with (-inf, -1); a document that shares no id with the query scores 0 and is a valid result.
 * tt_hybrid_scan_topk: the exact top-k by the hybrid score over documents 0 .. n_docs-1 for n_q (1 .. 64) queries, k 1 .. 1024, in
 *   ONE read of the store per pass of queries.  Every score is tt_lexical_score's out_hybrid for the same (query, document) with
 *   cand NULL, bit for bit: the lexical sum (lane l: the document's entries l, l + 64, ..., fmaf(q_w, d_w, acc), then the
 *   butterfly), the dense sum (lane l: elements 128 c + 2 l, + 1 for ascending c, bf16 operands converted to fp32, fmaf, the same
 *   butterfly) and the one mixing expression both kernels share -- so a score does not depend on n_q, on the other queries of the
 *   call, on the pass a query falls into, on where the document sits in the store, or on the wave that scored it.  The operands
 *   are tt_lexical_score's; q_dense [n_q][dim] and d_dense [n_docs][dim] bf16 are required.  After the call the workspace
 *   (tt_hybrid_scan_workspace_bytes: n_q rows of n_docs rounded up to 32 floats, tt_lexical_scan_workspace_bytes's rule) holds
 *   every score.  A tombstone (d_nnz < 0) writes NaN to its slot, which the selection never returns; neither its dense row nor its
 *   entries are read.  A live document with d_nnz == 0 scores the formula with lex = 0 and is a valid result.  Selection:
 *   tt_lexical_scan_topk's.  out_scores / out_idx [n_q][k], ordered by (score descending, document number ascending), padded with
 *   (-inf, -1); n_docs == 0 writes the padding without a scoring launch.  A persistent grid (three workgroups per compute unit) of
 *   four-wave workgroups; a wave owns whole documents, four consecutive numbers per step of a static grid-stride walk, loads each
 *   once into registers and scores it against every query of the pass; the pass's queries (entries and bf16 dense rows) are staged
 *   once per workgroup in LDS.  max_q_nnz_host (>= every q_nnz; the wrapper holds the lengths) sizes a query's slot: up to 64 ids,
 *   16 queries per pass (at most 40 KB of LDS); up to 512 ids, 8 per pass (at most 48 KB); the host launches one sweep per pass
 *   into the pass's own workspace rows.  Refused before a launch: dim not a multiple of 128 up to 1024, n_q outside 1 .. 64, k
 *   outside 1 .. 1024, max_q_nnz_host outside 0 .. 512 (TT_E_UNSUPPORTED); n_docs outside 0 .. INT_MAX, a null output, a negative
 *   weight or weights that sum to 0, and with n_docs > 0 a null q_dense, d_dense or array (TT_E_INVALID); a workspace that is NULL
 *   or too small (TT_E_WORKSPACE).  q_nnz and d_nnz are clamped in the kernel as tt_lexical_score clamps them (a q_nnz beyond
 *   max_q_nnz_host's class is cut to the class); the host wrapper (lexical.py) refuses a value outside. */
int tt_lexical_weights(const void* hidden, int n_rows, int ld, int H, const void* w, float bias_host, const int32_t* ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int max_len, int skip0_host, int skip1_host,
                       int skip2_host, int skip3_host, int32_t* out_terms, float* out_weights, int32_t* out_nnz, void* stream);
int tt_lexical_weights_f16(const void* hidden, int n_rows, int ld, int H, const void* w, float bias_host, const int32_t* ids,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int max_len, int skip0_host, int skip1_host,
                           int skip2_host, int skip3_host, int32_t* out_terms, float* out_weights, int32_t* out_nnz, void* stream);
int tt_lexical_weights_f32(const float* hidden, int n_rows, int ld, int H, const float* w, float bias_host, const int32_t* ids,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int max_len, int skip0_host, int skip1_host,
                           int skip2_host, int skip3_host, int32_t* out_terms, float* out_weights, int32_t* out_nnz, void* stream);
int tt_lexical_score(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                     const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, const int32_t* cand,
                     int n_cand, const void* q_dense, const void* d_dense, int dim, float w_dense, float w_lex, float* out_lex,
                     float* out_dense, float* out_hybrid, void* stream);
size_t tt_lexical_scan_workspace_bytes(int64_t n_docs, int n_q);
int tt_lexical_scan_topk(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                         const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, int64_t n_docs,
                         int k, float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);
size_t tt_hybrid_scan_workspace_bytes(int64_t n_docs, int n_q);
int tt_hybrid_scan_topk(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                        int max_q_nnz_host, const int32_t* d_terms, const float* d_weights, const int64_t* d_start,
                        const int32_t* d_nnz, int64_t n_docs, const void* q_dense, const void* d_dense, int dim, float w_dense,
                        float w_lex, int k, float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- Posting lists: an exact candidate generator for the lexical scan (csrc/postings.hip) --------------------------------------
 * tt_lexical_scan_topk scores every document for every query.  A document that shares no id with a query scores +0 (or is a
 * tombstone), so the only documents that can score above zero are those on the posting lists of the query's own ids.  These
 * entry points build such lists from the stores' CSR arrays and run the scan's own scoring kernel and the scan's own selection
 * over the union of chosen lists: what they return for a document is tt_lexical_scan_topk's bits.  WHICH lists to take, and whether
 * the candidates are known to hold the whole top-k, is the caller's decision (postings.py: thr_out > 0; MaxScore bounds from
 * term_ub) -- nothing here prunes.  All pointers are device memory.
 *
 * tt_postings_build: documents 0 .. n_sealed-1 of d_terms / d_weights / d_start (int64) / d_nnz (tt_lexical_score's arrays; d_nnz
 *   < 0: a tombstone, skipped whole; d_nnz clamped to 8192 as the scoring kernel clamps it) and a vocabulary size give
 *     post_off int64 [vocab + 1]   list t is post_doc[post_off[t] .. post_off[t + 1]); post_off[vocab] = the number of entries
 *     post_doc int32 [post_cap]    the documents holding id t, each once per occurrence, in NO specified order inside a list
 *     term_ub  fp32  [vocab]       the maximum over list t of the stored weights that are finite and >= 0; 0 for an empty list
 *     flags    int32 [1]           bit 0: a term outside [0, vocab) was met; bit 1: a weight that is negative, NaN or infinite;
 *                                  bit 2: a document whose ids are not strictly ascending (tt_lexical_score's precondition; a
 *                                  repeated id is scored once per occurrence, so term_ub would not bound its contribution)
 *   Histogram (integer atomicAdd per entry), exclusive scan, fill (the counts run back down: a slot per entry), per-term maximum
 *   (integer atomicMax on the bits of a non-negative float).  post_cap must be >= the live entries; the number of stored entries,
 *   live or dead, is such a bound.  The call synchronises the stream ONCE, after the scan, to read flags and the total: bit 0 or a
 *   total beyond post_cap fails it (TT_E_INVALID, tt_last_error) before anything is filled, and the fill writes no slot at or
 *   behind post_cap whatever the counters hold.  Bits 1 and 2 do not fail the build: either says term_ub bounds nothing (the caller
 *   must not prune; the lists themselves are complete, a repeated id lists its document once per occurrence).  Workspace: tt_postings_build_workspace_bytes (vocab counters).  vocab >= 1, n_sealed 0 .. INT_MAX - 64.
 * tt_lexical_topk_postings: for each of n_q (1 .. 64) queries, k 1 .. 1024 (anything else is refused before a launch, as
 *   tt_lexical_scan_topk refuses it), the caller lists ranges of post_doc: query q owns ranges r in [range_start[q],
 *   range_start[q + 1]) (int32 [n_q + 1]), range r is post_doc[range_lo[r] .. range_hi[r]) (int64, cut to [0, post_len); a listed
 *   document number outside [0, n_sealed) is ignored).  Per query:
 *     1. a bitmap of n_sealed bits is ORed from the ranges (integer atomicOr);
 *     2. it is compacted to an ASCENDING int32 list -- popcounts per span of TT_POSTINGS_SPAN documents, an exclusive scan, then
 *        every span writes from its own offset: no atomic decides a position, the list is a function of the bitmap alone;
 *     3. documents n_sealed .. n_docs-1 (the unsealed tail) are appended whole; cand_cnt_out[q] = the list's length;
 *     4. the list is scored by tt_lexical_score's kernel (a tombstone: NaN, as in the scan's workspace) and tt_lexical_scan_topk's
 *        selection picks the top k: out_scores / out_idx [n_q][k] ordered by (score descending, document number ascending),
 *        padded with (-inf, -1); thr_out[q] = the k-th best score or -inf when fewer than k candidates rank; cnt_out[q] = how
 *        many rank.
 *   The result equals tt_lexical_scan_topk's restricted to the listed documents and the tail, bit for bit; it equals the
 *   unrestricted one whenever every document outside the list scores below thr_out[q] (with ranges covering all of a query's
 *   ids: whenever thr_out[q] > 0).  grid_entries sizes the grids only (the longest sum of range lengths of any query, as far as
 *   the caller knows it; every walk is grid-strided, so any value gives the same output).  Workspace per query
 *   (tt_lexical_topk_postings_workspace_bytes): the bitmap, n_docs int32 candidates and n_docs fp32 scores.  n_docs 0 ..
 *   INT_MAX - 64, n_sealed 0 .. n_docs; n_docs == 0 writes the padding and thr_out -inf. */
#define TT_POSTINGS_SPAN 8192
size_t tt_postings_build_workspace_bytes(int vocab);
int tt_postings_build(const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, int64_t n_sealed,
                      int vocab, int64_t* post_off, int32_t* post_doc, int64_t post_cap, float* term_ub, int32_t* flags,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t tt_lexical_topk_postings_workspace_bytes(int64_t n_docs, int64_t n_sealed, int n_q);
int tt_lexical_topk_postings(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                             const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, int64_t n_docs,
                             const int32_t* post_doc, int64_t post_len, int64_t n_sealed, const int64_t* range_lo,
                             const int64_t* range_hi, const int32_t* range_start, int64_t grid_entries, int k, float* out_scores,
                             int32_t* out_idx, float* thr_out, int32_t* cnt_out, int32_t* cand_cnt_out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- Multi-vector head: BGE-M3's third head, late interaction at the model's own width (csrc/multivec.hip) ----------------------
 * BAAI/bge-m3 ships colbert_linear.pt (weight [dim][H], bias [dim]; dim = H = 1024): every token row but the first is projected,
 * biased and L2-normalised; mv(q, d) is the MEAN over the query's vectors of the maximum dot product with the document's.  The
 * late-interaction kernels above stop at dim 128, 128 query and 512 document rows, and have no bias; these are their wide forms.
 * All pointers are device memory; 16-bit operands are bf16 -- or fp16 for the `_f16` twins.
 *
 * tt_multivec_project: for n < n_out, y = W hidden[rows[n]] + bias (hidden [n_rows][ld], ld >= H a multiple of 8 elements (4 for
 *   `_f32`); W [dim][H]; bias fp32 [dim]; fp32 accumulation, the bias added to the fp32 sum), out[n] = y / max(||y||_2, 1e-12) in
 *   fp32 -- one division, one rounding to the output type; out [n_out][dim].  The squared norm is summed in fp32 in an order that
 *   depends on dim alone, so a row's bits depend neither on n_out, nor on its place in rows, nor on what else the launch holds.
 *   A row number outside [0, n_rows) gives a zero row (no bias); y = 0 gives 0.  H and dim each a multiple of 128 up to 1024
 *   (anything else is refused before a launch).  `_f32`: fp32 hidden states and fp32 W (the reference-precision paths) on the fp32
 *   MFMA, out in fp16 -- unit vectors fit fp16's range, and tt_maxsim_wide_f16 scores them.
 * tt_maxsim_wide: tt_maxsim's arguments and contract -- scores[q][c] = sum over i < q_len[q] of max over j < d_len[doc] of
 *   <Q[q_start[q] + i], D[d_start[doc] + j]>, doc = cand[q * n_cand + c] (cand NULL: doc = c); fp32 accumulation of exact 16-bit
 *   products; a token's maximum starts at -inf and rows past d_len are masked to -inf; the q_len maxima are added in index order
 *   in fp32; a negative candidate writes -inf, a document of length 0 scores 0; a score depends on its own pair alone -- plus
 *   `mean`: non-zero divides the sum by (float)q_len, one more rounding.  dim a multiple of 128 up to 1024 (refused otherwise);
 *   q_len 1 .. 512, d_len 0 .. 8192: the kernel clamps a length into its range, and the host wrapper (multivec.py), which holds
 *   the lengths, refuses one outside it.
 * tt_m3_mix: out[i] = (w_dense dense[i] + w_lex lex[i] + w_mv mv[i]) / (w_dense + w_lex + w_mv) for i < n, fp32; -inf in any input
 *   gives -inf.  Weights >= 0, finite and not all 0 (refused otherwise). */
int tt_multivec_project(const void* hidden, int n_rows, int ld, int H, const void* w, const float* bias, int dim, const int32_t* rows,
                        int n_out, void* out, void* stream);
int tt_multivec_project_f16(const void* hidden, int n_rows, int ld, int H, const void* w, const float* bias, int dim,
                            const int32_t* rows, int n_out, void* out, void* stream);
int tt_multivec_project_f32(const float* hidden, int n_rows, int ld, int H, const float* w, const float* bias, int dim,
                            const int32_t* rows, int n_out, void* out, void* stream);
int tt_maxsim_wide(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs, const int64_t* d_start,
                   const int32_t* d_len, const int32_t* cand, int n_cand, int dim, int mean, float* scores, void* stream);
int tt_maxsim_wide_f16(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs,
                       const int64_t* d_start, const int32_t* d_len, const int32_t* cand, int n_cand, int dim, int mean, float* scores,
                       void* stream);
int tt_m3_mix(const float* dense, const float* lex, const float* mv, int64_t n, float w_dense, float w_lex, float w_mv, float* out,
              void* stream);

/* ---- SPLADE: learned sparse vectors from a masked-language-model head (csrc/splade.hip) ------------------------------------------
 * A SPLADE checkpoint is a BertForMaskedLM; a text's weight for vocabulary id v is max over its tokens t of
 * log1p(relu(logit[t][v])), so a text activates ids it does not contain.  The logits ([rows][vocabulary]: 61 KB per token for
 * BERT-base in bf16) are never written: the vocabulary projection and the maximum over a sequence's rows are one kernel.  What comes
 * out is what the lexical kernels above take: ascending (id, weight) entries.  All pointers are device memory; 16-bit operands are
 * bf16 -- or fp16 for the `_f16` twin.
 *
 * tt_splade_pool: t [n_rows][ld] (ld >= H, a multiple of 8 elements) holds the TRANSFORMED hidden states -- the rows after the head's
 *   dense -> GELU -> LayerNorm, which the caller computes with tt_gemm_* (epilogue 1) and tt_layernorm_* -- E [Vp][H] the decoder
 *   matrix in the same type, bias fp32 [Vp], out fp32 [n_seq][ldo] with ldo >= Vp.  For sequence b and column v < Vp, with
 *     m = max over the rows r in [seq_start[b], seq_start[b] + seq_len[b]) and in [0, n_rows) of (fp32 sum_k t[r][k] E[v][k]),
 *     activation 0:  out[b][v] = m + bias[v]
 *     activation 1:  out[b][v] = log1pf(max(0, m + bias[v]))
 *   (columns Vp .. ldo-1 are not written).  The bias is added after the maximum, and relu and log1p applied once per column: fp32
 *   rounding, relu and log1p are monotone, so these are the bits of applying them to every row first.  A sequence with no rows
 *   (length <= 0, a negative start, a start >= n_rows) writes -inf under activation 0 and 0 under activation 1; a seq_len beyond
 *   max_len is clamped to it.  A row's fp32 sum is ONE chain of mfma_f32_16x16x32 over k = 0, 32, .. H-32 from a zero accumulator: it
 *   depends on H alone -- not on the row's place in its sequence, nor on whether the sequence fills one pass of 64 rows or several --
 *   and the maximum is exact, associative and commutative.  A sequence's output is therefore the same bits alone or in any batch,
 *   at any start row, in any launch geometry.  Non-finite hidden states, as built: the maximum is fmaxf's, which passes over a NaN,
 *   so a row whose sum for a column is NaN takes no part in that column (if every row's is, the column is that of a sequence with no
 *   rows); a sum of +inf wins and gives +inf under either activation; a NaN never reaches another sequence.  A NaN bias gives NaN
 *   under activation 0 and 0 under activation 1.  H a multiple of 128 up to 1024, Vp a multiple of 128 up to 65536, max_len
 *   1 .. 8192, n_seq up to 65535: anything else is refused before a launch (TT_E_UNSUPPORTED).
 * tt_sparse_compact: w fp32 [n_seq][ldw], V <= ldw the true vocabulary size (ids >= V -- a loader's padding -- are never read).  Row
 *   b's entries with w > 0 are kept (decided on the bits: a denormal is kept, a NaN, a zero of either sign and a negative are not);
 *   if more than max_terms qualify, the max_terms largest by (weight descending, id ascending) -- sentence-transformers'
 *   max_active_dims.  out_terms[b * max_terms ..] holds the kept ids in ASCENDING order, out_weights their weights (unchanged bits),
 *   out_nnz[b] their number; the slots behind them hold (-1, 0).  That is tt_lexical_score's precondition.  Deterministic: the only
 *   atomics are integer histogram counts, whose order of arrival does not show.  V 1 .. 65536, max_terms 1 .. 8192 (refused
 *   otherwise). */
int tt_splade_pool(const void* t, int n_rows, int ld, int H, const void* E, const float* bias, int Vp, const int32_t* seq_start,
                   const int32_t* seq_len, int n_seq, int max_len, int activation, float* out, int ldo, void* stream);
int tt_splade_pool_f16(const void* t, int n_rows, int ld, int H, const void* E, const float* bias, int Vp, const int32_t* seq_start,
                       const int32_t* seq_len, int n_seq, int max_len, int activation, float* out, int ldo, void* stream);
int tt_sparse_compact(const float* w, int ldw, int V, int n_seq, int max_terms, int32_t* out_terms, float* out_weights, int32_t* out_nnz,
                      void* stream);

/* Per-kernel device timing (HIP events on the launch stream), for bench.py's roofline leg.
 * tt_prof_enable(1) (or a mask of 1 << id, to time only some kernels) starts recording one event pair per launch of the tracked kernels on the
 * calling thread; tt_prof_read() synchronises those events and returns total milliseconds
 * and launch count for kernel id `which` since the last enable, then keeps recording.
 * ids: 1 scan filter pass, 2 scan sample pass, 3 top-k select, 4 gemm, 5 attention, 6 row ops,
 * 7 scan tail rows (the < 256 rows behind the tiled filter pass of a 65+ query batch) */
int tt_prof_enable(int on);
int tt_prof_read(int which, double* total_ms_host, int* launches_host);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* TT_HIP_H */
