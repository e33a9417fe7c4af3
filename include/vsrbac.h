/*
 * vsrbac.h — C ABI of libvsrbac: RBAC-filtered k-NN on AMD Instinct MI355X (gfx950).
 *
 * Drop-in boundary for ONE path of rjzhb/VectorSearch-RBAC: "distance(query, corpus rows) AND
 * permission(user, row) -> top-k", which the reference runs inside PostgreSQL through pgvector
 * (file:line below are relative to the reference tree):
 *
 *   pgvector/src/vector.c:549-563,568-594   VectorL2SquaredDistance, l2_distance, vector_l2_squared_distance
 *   pgvector/src/vector.c:596-636           VectorInnerProduct, inner_product, vector_negative_inner_product
 *   pgvector/src/vector.c:638-685           VectorCosineSimilarity, cosine_distance
 *   pgvector/src/vector.c:714-739           VectorL1Distance, l1_distance
 *   pgvector/src/hnswscan.c:179-316         hnswgettuple   (first call runs the whole search; later calls pop TIDs)
 *   pgvector/src/ivfscan.c:339-389          ivfflatgettuple (same contract)
 *   controller/baseline/pg_row_security/row_level_security.py:54-65   RLS policy = the per-row permission test
 *   controller/baseline/prefilter/initialize_partitions.py:281-311    role tables  = pre-filter row sets
 *   controller/dynamic_partition/search.py:54-58,347-364              comb_role -> partitions, merge + dedup
 *
 * A PostgreSQL extension shim keeps pgvector's SQL surface (type vector, operators
 * <-> <#> <=> <+>, access methods hnsw / ivfflat, GUC names) and calls these entry points; the Python
 * harness mirror (vectorsearch-rbac_amd/vsrbac) binds them with ctypes.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++ or torch types; every function returns a vsr_status (0 = ok)
 *     unless stated; never throws, never exits.  vsr_last_error() gives the message of the last failure
 *     on the calling thread (dimension mismatch keeps pgvector's text, vector.c:60-67).
 *   - host pointers are borrowed for the duration of the call; the library owns all device memory.
 *   - "_device" variants take device pointers and enqueue on the context's stream without synchronising.
 *   - a context is bound to one GPU and one host thread at a time; open one context per process after
 *     fork (PostgreSQL backends), never share across fork.  A corpus, its filters and every session searching it
 *     (vsr_search_device_on) belong to ONE host thread at a time too: the planner keeps scratch marks in the filters.
 *   - there is no CPU fallback: without a usable gfx950 device vsr_open fails with VSR_ERR_NO_DEVICE.
 */
#ifndef VSRBAC_H
#define VSRBAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSR_ABI_VERSION 2

typedef struct vsr_ctx vsr_ctx;
typedef struct vsr_corpus vsr_corpus;
typedef struct vsr_filter vsr_filter;

typedef enum {
    VSR_OK = 0,
    VSR_ERR_INVALID = 1,        /* bad argument */
    VSR_ERR_DIM_MISMATCH = 2,   /* "different vector dimensions %d and %d" (vector.c:60-67) */
    VSR_ERR_NO_DEVICE = 3,      /* no gfx950 GPU / HIP runtime unusable */
    VSR_ERR_HIP = 4,            /* a HIP call failed; see vsr_last_error() */
    VSR_ERR_OOM = 5,
    VSR_ERR_UNSUPPORTED = 6,    /* e.g. k > VSR_MAX_K */
    VSR_ERR_NO_RBAC = 7         /* filter requested before vsr_rbac_load */
} vsr_status;

/* operator of pgvector/sql/vector.sql:174-192; the value returned is the operator's float8 result */
typedef enum {
    VSR_METRIC_L2 = 0,          /* <->  sqrt(sum (a-b)^2)            */
    VSR_METRIC_IP = 1,          /* <#>  -sum a*b                     */
    VSR_METRIC_COSINE = 2,      /* <=>  1 - clamp(cos(a,b)), NaN for a zero vector (sorted last) */
    VSR_METRIC_L1 = 3,          /* <+>  sum |a-b|                    */
    /* pgvector's type bit (sql/vector.sql: <~>, <%>); accepted by the *_bit entry points only */
    VSR_METRIC_HAMMING = 4,     /* <~>  popcount(a ^ b)              */
    VSR_METRIC_JACCARD = 5      /* <%>  |a&b| == 0 ? 1 : 1 - |a&b| / (double) (|a| + |b| - |a&b|)   (bitutils.c:96-129) */
} vsr_metric;

/* how a permission set is applied to the scan */
typedef enum {
    VSR_FILTER_RANGES = 0,      /* pre-filter: only the permitted row ranges are read (role / partition tables) */
    VSR_FILTER_BITMAP = 1       /* post-filter: whole-corpus scan order, per-row permission bit tested in the
                                   distance loop (row-level security); fully masked tiles are skipped */
} vsr_filter_mode;

#define VSR_MAX_K 2048

/* ---- context -------------------------------------------------------------------------------- */
int         vsr_abi_version(void);
const char* vsr_last_error(void);
const char* vsr_status_string(int status);

int vsr_open(int device_ordinal, vsr_ctx** out);
int vsr_close(vsr_ctx* ctx);
/* use the caller's HIP stream (hipStream_t as void*, e.g. torch's current stream); NULL = the context's own
 * non-blocking stream.  HIP's null stream has the handle 0 as well: name it as VSR_STREAM_NULL (= hipStreamLegacy). */
#define VSR_STREAM_NULL ((void*) 1)
int vsr_set_stream(vsr_ctx* ctx, void* hip_stream);
int vsr_synchronize(vsr_ctx* ctx);
int vsr_device_info(vsr_ctx* ctx, char* name, int name_len, int* compute_units, int64_t* hbm_bytes);

/* ---- corpus: resident row-major fp32 rows + row identity -------------------------------------- */
/* rows[n][dim]; block_ids[n] / doc_ids[n] identify a row as (document_id, block_id) like the reference's
 * documentblocks table (controller/initialize_main_tables.py:54-61); either may be NULL (block_id = row
 * index, document_id = 0).  Rows are re-ordered internally by (document_id, block_id); results report the
 * caller's row index.  row_offset is added to internal rows in raw keys (multi-GPU shards; 0 otherwise). */
int vsr_corpus_load(vsr_ctx* ctx, const float* rows, int64_t n, int dim,
                    const int64_t* block_ids, const int32_t* doc_ids, int64_t row_offset,
                    vsr_corpus** out);
/* pgvector's halfvec (halfvec.h; HALFVEC_MAX_DIM 16000): rows[n][dim] IEEE binary16 bit patterns.  Everything else as
 * vsr_corpus_load.  The rows stay binary16 on the device (2 bytes per element, plus |row|^2): no fp32 image, no
 * screening planes -- the rows are their own (K2h).  Every distance is pgvector's for the type (halfutils.c): both operands widened to fp32, then the
 * arithmetic of vector.c -- so queries stay const float*, and the library rounds every query element to binary16 (round to
 * nearest even, Float4ToHalf) and widens it again first, which is what `ORDER BY col <-> $1::halfvec` computes.  vsr_search
 * refuses a finite query element that rounds to +-Inf (|v| >= 65520) with VSR_ERR_INVALID,
 * `"<v>" is out of range for type halfvec`; the device entry points do not look, the element becomes +-Inf.  A dimension
 * mismatch reads "different halfvec dimensions %d and %d".  All metrics, filters, RBAC, k <= VSR_MAX_K, raw keys and the
 * shard merge work as for any corpus.  Passes that several queries share (L2 / inner product / cosine, dim >= 61) are
 * screened on the f16 matrix cores and re-ranked exactly, as over an fp32 corpus: vsr_search_device may return flagged
 * queries (negative counts), vsr_search and vsr_search_device_exact re-run them, on the exact kernel over the half rows.
 * vsr_set_screening(ctx, 0) keeps every search on that kernel; vsr_set_query_hint has no effect.  Non-finite rows are accepted as for fp32 (pgvector rejects them on input): NaN
 * distances sort last.  The HNSW opclasses halfvec_l2_ops / halfvec_ip_ops / halfvec_cosine_ops are vsr_hnsw_load_half /
 * vsr_hnsw_build_half below, searched by the float vsr_hnsw_search* entry points (K4h); vsr_hnsw_load and vsr_hnsw_build* over
 * such a corpus keep answering VSR_ERR_UNSUPPORTED, the message names the halfvec corpus and those entry points.  The IVFFlat
 * opclasses are vsr_ivf_kmeans_half / vsr_ivf_assign_half / vsr_ivf_load_half below (K3h); vsr_ivf_load and vsr_ivf_assign over such
 * a corpus keep answering VSR_ERR_UNSUPPORTED, the message names the halfvec corpus and the _half entry points. */
int vsr_corpus_load_half(vsr_ctx* ctx, const uint16_t* rows, int64_t n, int dim,
                         const int64_t* block_ids, const int32_t* doc_ids, int64_t row_offset,
                         vsr_corpus** out);
int     vsr_corpus_is_half(const vsr_corpus* corpus);        /* 1 / 0 */
/* pgvector's bit (bitvec.c, bitutils.c; what binary_quantize(vector | halfvec) returns, vector.c:941-968): rows[n][(dim + 7) / 8]
 * bytes, tightly packed, in PostgreSQL's varbit order -- element i is bit 7 - i % 8 of byte i / 8.  dim counts bits, 1 .. 64000
 * (HNSW_MAX_DIM * 32, the widest bit column a pgvector index takes, hnswutils.c:1403), anything else VSR_ERR_INVALID.  Bits past
 * dim in the last byte are IGNORED: the library clears them on load and on query staging (varbit guarantees zero padding and
 * pgvector relies on it; this library does not).  Everything else as vsr_corpus_load.  The rows stay packed on the device (16
 * bytes per 128 bits, plus the row's popcount): no fp32 image, no norms, no planes, no class view.
 * Searches go through vsr_search_bit / vsr_search_bit_device(_on), which are vsr_search / vsr_search_device(_on) with queries of
 * (dim + 7) / 8 packed bytes (device queries need no alignment) and metric VSR_METRIC_HAMMING or VSR_METRIC_JACCARD.  out_dist is
 * (float) of the operator's float8: a Hamming distance is an integer <= 64000 and exact in fp32; Jaccard is evaluated in double
 * as bitutils.c does and then rounded, the way cosine is.  Order: ((float) distance ascending, document_id, block_id), as
 * everywhere; keys are monotone(fp32) << 32 | global row, so vsr_merge_topk_* work untouched.  Rounding to fp32 is monotone: it
 * can only merge two distinct float8 Jaccard values into a tie (then broken by the ids), never reorder them -- and not even
 * that below 2049 dimensions, where two distinct fractions with denominators <= 2048 differ by more than an fp32 ulp.
 * The scan is exact by construction (integer popcounts, K1b): nothing is screened, no query is ever flagged, counts are never
 * negative, vsr_set_screening / vsr_set_query_hint have no effect.  All filters (vsr_rbac_load, the four vsr_filter_*
 * constructors, both modes), k <= VSR_MAX_K, row_offset, sessions, raw keys, the shard merge, vsr_stats_get (scan_bytes counts
 * (dim + 7) / 8 bytes per row) and vsr_corpus_device_bytes work as for any corpus.
 * Errors.  A dimension mismatch is VSR_ERR_DIM_MISMATCH, "different bit lengths %u and %u" with the column's length first
 * (CheckDims, bitvec.c:32-39).  vsr_search_bit* on a corpus that is not a bit corpus, or with a metric other than 4 / 5:
 * VSR_ERR_INVALID.  vsr_search*, vsr_ivf_load, vsr_ivf_assign, vsr_hnsw_load and vsr_hnsw_build* over a bit corpus:
 * VSR_ERR_UNSUPPORTED, the message names the bit corpus.  The HNSW opclasses bit_hamming_ops / bit_jaccard_ops are
 * vsr_hnsw_load_bit / vsr_hnsw_build_bit / vsr_hnsw_search_bit* below; the IVFFlat opclass bit_hamming_ops is vsr_ivf_kmeans_bit /
 * vsr_ivf_assign_bit / vsr_ivf_load_bit / vsr_ivf_probe_bit / vsr_ivf_search_bit* below (K3b) -- vsr_ivf_load and vsr_ivf_assign keep
 * their refusal of a bit corpus, whose message predates those entry points.  The float entry points keep rejecting metrics 4 / 5
 * with VSR_ERR_INVALID. */
int vsr_corpus_load_bit(vsr_ctx* ctx, const uint8_t* rows, int64_t n, int dim,
                        const int64_t* block_ids, const int32_t* doc_ids, int64_t row_offset,
                        vsr_corpus** out);
int     vsr_corpus_is_bit(const vsr_corpus* corpus);         /* 1 / 0 */
/* binary_quantize over the RESIDENT rows of an fp32 or halfvec corpus, on the device: a new bit corpus of the same dim whose bit
 * i is set where element i > 0 (a widened half is positive exactly when the half is).  Same context, same row identity
 * (block / document ids, caller row indices, row_offset), same internal order.  RBAC tables are NOT inherited: run vsr_rbac_load
 * on the new corpus.  The new corpus is independent of src (free either first).  src a bit corpus or an index view:
 * VSR_ERR_INVALID. */
int vsr_corpus_binary_quantize(vsr_corpus* src, vsr_corpus** out);
/* pgvector's sparsevec (sparsevec.c, sparsevec.h): n rows as CSR -- indptr[n + 1] (row i owns entries indptr[i] .. indptr[i + 1]),
 * indices[nnz] zero-based, values[nnz] fp32.  Validated as sparsevec_recv validates a value (sparsevec.c:53-133, 493-539), every
 * refusal VSR_ERR_INVALID in pgvector's words: dim 1 .. 1000000000; at most 16000 non-zeros per row and no more than dim; indices in
 * range, ascending, no duplicates; no NaN, no Inf, no stored zero.  Empty rows are legal.  Identity arrays, row_offset and the
 * (document_id, block_id) internal order are vsr_corpus_load's; the CSR rows are permuted on the host.  Resident form: interleaved
 * (index, value) entries of 8 bytes (rows padded to an even entry count), 8 bytes of row offset and |row|^2 per row: no dense
 * image, no planes, no class view.
 * Searches go through vsr_search_sparse / vsr_search_sparse_device(_on): metrics VSR_METRIC_L2 .. VSR_METRIC_L1, the operators <->,
 * <#>, <=>, <+> of sparsevec.c:803-1037, exact (nothing is screened, nothing flags), ordered as every search is.  Sums are fp32 as
 * pgvector's are, in another order; the query terms no row entry meets enter as (float) of a double difference.
 * vsr_search*, vsr_search_bit*, vsr_search_quantized*, vsr_corpus_binary_quantize, vsr_ivf_load, vsr_ivf_assign, vsr_hnsw_load
 * and vsr_hnsw_build(_ex) over a sparse corpus: VSR_ERR_UNSUPPORTED, the message names sparsevec.  The HNSW opclasses
 * sparsevec_l2_ops / sparsevec_ip_ops / sparsevec_cosine_ops / sparsevec_l1_ops are vsr_hnsw_load_sparse / vsr_hnsw_build_sparse /
 * vsr_hnsw_search_sparse* below (K4s); pgvector has no IVFFlat opclass for sparsevec.  (The text of vsr_hnsw_load's and
 * vsr_hnsw_build's refusal still says the type "has no index path yet": it is kept as it was.) */
int vsr_corpus_load_sparse(vsr_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n, int dim,
                           const int64_t* block_ids, const int32_t* doc_ids, int64_t row_offset,
                           vsr_corpus** out);
int     vsr_corpus_is_sparse(const vsr_corpus* corpus);      /* 1 / 0 */
/* device bytes holding VECTOR data of any corpus: rows, norms, every screening plane and, once vsr_rbac_load has built it,
 * the class-ordered copy of the int8 planes; identity arrays, RBAC tables and filters excluded */
int64_t vsr_corpus_device_bytes(const vsr_corpus* corpus);
int     vsr_corpus_free(vsr_corpus* corpus);
int64_t vsr_corpus_rows(const vsr_corpus* corpus);
int     vsr_corpus_dim(const vsr_corpus* corpus);

/* ---- RBAC tables (UserRoles, PermissionAssignment of controller/initialize_main_tables.py:17-72) ----
 * Drops the filters the corpus cached for the previous tables.  A corpus with int8 planes (integer 0..255 rows, d <= 128) also gets a copy of those
 * planes in permission-class order here (~137 bytes per row) unless its context was opened under VSR_NO_CLASS_VIEW=1 or the
 * memory is not there; searches never depend on it. */
int vsr_rbac_load(vsr_corpus* corpus,
                  const int32_t* ur_user, const int32_t* ur_role, int64_t n_user_roles,
                  const int32_t* pa_role, const int32_t* pa_doc, int64_t n_permissions);

/* ---- filters ----------------------------------------------------------------------------------- */
/* rows visible to the user: EXISTS role in UserRoles(user): (role, document) in PermissionAssignment.
 * Cached per role combination and mode; owned by the corpus (do not free). */
int vsr_filter_for_user(vsr_corpus* corpus, int32_t user_id, int mode, vsr_filter** out);
int vsr_filter_for_roles(vsr_corpus* corpus, const int32_t* role_ids, int n_roles, int mode, vsr_filter** out);
/* byte-per-row mask in the caller's row order (uint8 allowed_mask[N] of global_hnsw_index.cpp:136-183,
 * char filter map of acorn_benchmark/src/benchmark_utils.cpp:342-396).  Caller frees with vsr_filter_free. */
int vsr_filter_from_bytemask(vsr_corpus* corpus, const uint8_t* allowed, int mode, vsr_filter** out);
/* a dynamic partition = a set of documents (load_result_to_database.py:207-240); user_id >= 0 adds the
 * per-row permission test of an "impure" partition (load_result_to_database.py:590-624), -1 = pure. */
int vsr_filter_from_documents(vsr_corpus* corpus, const int32_t* doc_ids, int64_t n_docs, int32_t user_id,
                              vsr_filter** out);
int     vsr_filter_free(vsr_filter* filter);
int64_t vsr_filter_allowed_rows(const vsr_filter* filter);   /* rows that pass the filter */
int64_t vsr_filter_scanned_rows(const vsr_filter* filter);   /* rows whose distance work is priced (N for bitmap mode) */

/* ---- search -------------------------------------------------------------------------------------- */
/* nq queries of `dim` floats; filters[i] applies to query i (filters == NULL or filters[i] == NULL: no filter).
 * Outputs are nq*k, row-major, ordered by (distance asc, NaN last, document_id asc, block_id asc); entries
 * past out_counts[i] hold id -1 and +Inf.  out_rows (caller row index) and out_doc_ids may be NULL. */
int vsr_search(vsr_corpus* corpus, const float* queries, int nq, int dim, int k, int metric,
               const vsr_filter* const* filters,
               int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows,
               float* out_dist, int32_t* out_counts);

/* vsr_search over a bit corpus (vsr_corpus_load_bit): queries[nq][(dim + 7) / 8] packed bytes, dim in bits, metric
 * VSR_METRIC_HAMMING / VSR_METRIC_JACCARD */
int vsr_search_bit(vsr_corpus* corpus, const uint8_t* queries, int nq, int dim, int k, int metric,
                   const vsr_filter* const* filters,
                   int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows,
                   float* out_dist, int32_t* out_counts);

/* same, queries and outputs in device memory, enqueued on the context's stream, no synchronisation.
 * out_keys (nq*k, may be NULL) receives the raw ordering keys (monotone fp32 distance << 32 | global row)
 * that vsr_merge_topk_device consumes. */
int vsr_search_device(vsr_corpus* corpus, const float* d_queries, int nq, int dim, int k, int metric,
                      const vsr_filter* const* filters,
                      int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                      float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);

/* same, in the stream and workspaces of `session`: another context opened on the corpus's device (NULL = the corpus's
 * own).  Two sessions let two batches over one corpus be in flight at once, so the small selection / re-rank kernels of
 * one batch run under the scan launch of the other (a serving loop alternates sessions; bench.py does).  Flags and
 * statistics (vsr_screening_check, vsr_stats_get) are per session.  vsr_corpus_free / vsr_filter_free wait for the
 * corpus's own context only: vsr_synchronize every other session that searched the corpus before freeing it. */
int vsr_search_device_on(vsr_ctx* session, vsr_corpus* corpus, const float* d_queries, int nq, int dim, int k, int metric,
                         const vsr_filter* const* filters,
                         int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                         float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);

/* vsr_search_device / vsr_search_device_on over a bit corpus; d_queries needs no alignment.  Never flags. */
int vsr_search_bit_device(vsr_corpus* corpus, const uint8_t* d_queries, int nq, int dim, int k, int metric,
                          const vsr_filter* const* filters,
                          int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                          float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);
int vsr_search_bit_device_on(vsr_ctx* session, vsr_corpus* corpus, const uint8_t* d_queries, int nq, int dim, int k, int metric,
                             const vsr_filter* const* filters,
                             int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                             float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);

/* vsr_search over a sparse corpus (vsr_corpus_load_sparse): nq queries as CSR (q_indptr[nq + 1], q_indices zero-based, q_values),
 * validated as rows are (VSR_ERR_INVALID, pgvector's words); an empty query is legal.  dim other than the corpus's:
 * VSR_ERR_DIM_MISMATCH, "different sparsevec dimensions %d and %d" (CheckDims, sparsevec.c), the column's first.  A corpus that is
 * not sparse: VSR_ERR_INVALID. */
int vsr_search_sparse(vsr_corpus* corpus, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq,
                      int dim, int k, int metric, const vsr_filter* const* filters,
                      int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows,
                      float* out_dist, int32_t* out_counts);
/* vsr_search_device / vsr_search_device_on over a sparse corpus: the three CSR arrays of the queries in device memory.  They are
 * not read on the host, so the caller states max_query_nnz, the largest number of non-zeros of any query of the call
 * (0 .. 16000): it sizes the queries' lookup tables.  A query with more entries than that (or with a negative count) is not
 * staged -- it is searched as an empty query -- and sets a bit of the session's guard word: vsr_screening_check then fails.
 * Entries whose index is not in 0 .. dim - 1 are dropped the same way.  Never flags. */
int vsr_search_sparse_device(vsr_corpus* corpus, const int64_t* d_q_indptr, const int32_t* d_q_indices, const float* d_q_values,
                             int nq, int dim, int max_query_nnz, int k, int metric, const vsr_filter* const* filters,
                             int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                             float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);
int vsr_search_sparse_device_on(vsr_ctx* session, vsr_corpus* corpus, const int64_t* d_q_indptr, const int32_t* d_q_indices,
                                const float* d_q_values, int nq, int dim, int max_query_nnz, int k, int metric,
                                const vsr_filter* const* filters,
                                int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                                float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);

/* ---- two-stage search: Hamming shortlist on the bits, exact re-rank on the source rows ------------------------------
 *   SELECT * FROM (SELECT * FROM items ORDER BY binary_quantize(embedding)::bit(n) <~> binary_quantize($1) LIMIT shortlist)
 *   ORDER BY embedding <op> $1 LIMIT k;             (pgvector README, "Re-rank by the original vectors for better recall")
 * `bits` must be the corpus vsr_corpus_binary_quantize made from `source` (fp32 or halfvec; either may still be freed first,
 * and a source freed and loaded again is another corpus).  Per query q of `dim` floats:
 *   1. qb = binary_quantize(q): bit i set where q[i] > 0, from the fp32 value as given, also for a halfvec source;
 *   2. S = the answer of vsr_search_bit(bits, qb, k = shortlist, VSR_METRIC_HAMMING, filters[i]): the `shortlist` nearest
 *      permitted rows by (Hamming, document_id, block_id), fewer if the filter admits fewer.  The filters are filters of
 *      `bits`, the corpus that is scanned (RBAC tables are not inherited by a quantized corpus);
 *   3. the exact operator distance of q to the SOURCE rows of S, in the arithmetic vsr_search reports (halfvec source: q
 *      rounded to binary16 and widened); the first min(k, |S|) by (distance asc, NaN last, document_id, block_id) are the
 *      answer, entries past out_counts[i] hold -1 / +Inf (out_keys: all ones).
 * So a filter admitting at most `shortlist` rows gives exactly vsr_search(source) over the same rows, and the shortlists of one
 * query are nested: recall against the exact search never decreases as `shortlist` grows.  Deterministic; no query is ever
 * flagged, counts are never negative, vsr_set_screening and vsr_set_query_hint have no effect.  out_rows and out_doc_ids may be
 * NULL.  k <= shortlist <= VSR_MAX_K; metric L2, inner product or cosine.
 * Errors.  VSR_ERR_INVALID: source a bit corpus or an index view, bits not a bit corpus, bits not made from source (the message
 * names both corpora), k < 1, shortlist < k, shortlist > VSR_MAX_K, a metric other than 0 .. 3, a filter of another corpus
 * (source's included), and -- host entry point, halfvec source -- a finite query element that overflows binary16, as vsr_search.
 * VSR_ERR_UNSUPPORTED: VSR_METRIC_L1.  VSR_ERR_DIM_MISMATCH: dim is not the source's, in vsr_search's words for that corpus. */
int vsr_search_quantized(vsr_corpus* source, vsr_corpus* bits, const float* queries, int nq, int dim, int k, int shortlist,
                         int metric, const vsr_filter* const* filters,
                         int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows,
                         float* out_dist, int32_t* out_counts);
/* same, queries (nq x dim floats, row stride dim, 4-byte aligned) and outputs in device memory: both stages are enqueued on
 * the stream of `session` (NULL, or vsr_search_quantized_device: the bits corpus's own context; the session must be on the
 * corpora's device) with no synchronisation and no host round trip in between.  d_out_keys (nq*k, may be NULL): monotone
 * fp32 distance << 32 | global row (row_offset included), as vsr_search_device's.  Query elements are not range-checked. */
int vsr_search_quantized_device(vsr_corpus* source, vsr_corpus* bits, const float* d_queries, int nq, int dim, int k,
                                int shortlist, int metric, const vsr_filter* const* filters,
                                int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                                float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);
int vsr_search_quantized_device_on(vsr_ctx* session, vsr_corpus* source, vsr_corpus* bits, const float* d_queries, int nq,
                                   int dim, int k, int shortlist, int metric, const vsr_filter* const* filters,
                                   int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                                   float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys);

/* same as vsr_search_device_on, but the call returns only when every query is PROVEN exact: it waits for the search,
 * and queries the screening flagged (below) are re-run on the exact path and patched into the outputs, all on the
 * session's stream.  n_rerun (may be NULL) receives how many queries that took.  Synchronises the session's stream. */
int vsr_search_device_exact(vsr_ctx* session, vsr_corpus* corpus, const float* d_queries, int nq, int dim, int k, int metric,
                            const vsr_filter* const* filters,
                            int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                            float* d_out_dist, int32_t* d_out_counts, uint64_t* d_out_keys, int32_t* n_rerun);

/* Flagged queries.  Shared passes of L2 / inner-product / cosine searches may run on the matrix cores: a bf16 / fp32
 * MFMA screening with sampled thresholds keeps 2k candidates per query and an exact re-rank reports the k best (see
 * DESIGN.md, K2w / K5r).  The re-rank FLAGS a query when the screening's rounding error or a too-tight threshold could
 * have excluded a true result (rare: none in the benchmark's 3 M queries).  A flagged query cannot be mistaken for a
 * result: its out_counts entry is NEGATIVE (-1 - rows written).  vsr_search and vsr_search_device_exact re-run
 * flagged queries themselves.  After the asynchronous vsr_search_device(_on) the caller either tests the counts on the
 * device or calls vsr_screening_check: flagged_total = flagged queries since vsr_open, flags_last_call[i] != 0 =
 * query i of the last call must be re-run with screening disabled.  vsr_screening_check synchronises. */
/* Queries of a SIFT-like workload: a corpus whose elements are all integers 0..255 (d <= 128) also keeps int8 planes, and
 * L2 searches whose QUERIES are such integers too screen on them (a quarter of the fp32 bytes per row).  Host queries
 * (vsr_search) are checked by the library.  For device-resident queries the caller states it: u8_queries != 0 promises
 * that the queries of this context's vsr_search_device calls are integer-valued in 0..255.  The promise is verified on
 * the device: a query that breaks it is FLAGGED (re-run like any flagged query) and the hint is dropped. */
int vsr_set_query_hint(vsr_ctx* ctx, int u8_queries);
int vsr_set_screening(vsr_ctx* ctx, int enable);           /* default: enabled; 0 also disables threshold seeding, so
                                                              searches of that context are exact and never flag */
int vsr_screening_check(vsr_ctx* ctx, int64_t* flagged_total, int32_t* flags_last_call, int nq);

/* merge n_parts per-shard results (layout [n_parts][nq][k], as all-gathered from vsr_search_device) into the
 * global top-k: the client-side merge of search.py:347-364 done on the GPU.  Every part's list is sorted by key with
 * KEY_EMPTY (all ones; payload -1 / -1 / +Inf) after its real entries.  Keys must be UNIQUE across the parts of a query
 * (disjoint shards: the global row in the low 32 bits makes them so); the kernel does not remove duplicates -- replicated
 * partitions are deduplicated on the host (vsrbac/placement.py).  n_parts * k <= 8192, else VSR_ERR_UNSUPPORTED.
 * d_out_keys (nq*k, may be NULL) receives the merged keys, KEY_EMPTY past the count. */
int vsr_merge_topk_device(vsr_ctx* ctx, const uint64_t* d_keys, const int64_t* d_block_ids,
                          const int32_t* d_doc_ids, const float* d_dist, int n_parts, int nq, int k,
                          int64_t* d_out_block_ids, int32_t* d_out_doc_ids, float* d_out_dist,
                          uint64_t* d_out_keys, int32_t* d_out_counts);

/* Same merge for PACKED per-shard results: one record per shard of vsr_packed_result_bytes(nq, k) = nq*k*24 bytes,
 * laid out {keys u64[nq][k], block_ids i64[nq][k], doc_ids i32[nq][k], dist f32[nq][k]} — i.e. the four output
 * pointers of vsr_search_device aimed into one buffer — so that ONE all-gather moves a rank's whole result. */
int64_t vsr_packed_result_bytes(int nq, int k);
int vsr_merge_topk_packed_device(vsr_ctx* ctx, const void* d_packed, int n_parts, int nq, int k,
                                 int64_t* d_out_block_ids, int32_t* d_out_doc_ids, float* d_out_dist,
                                 uint64_t* d_out_keys, int32_t* d_out_counts);

/* operator value for n explicit pairs a[i] (dim floats) vs b[i] (or one shared b when b_broadcast != 0):
 * what `SELECT a <-> b` evaluates per row (vector.c:568-578 etc.), batched.  Host pointers. */
int vsr_pair_distances(vsr_ctx* ctx, int metric, const float* a, const float* b, int64_t n_pairs,
                       int dim_a, int dim_b, int b_broadcast, double* out);

/* hamming_distance / jaccard_distance (bitvec.c:46-77) for n explicit pairs of bit strings, (dim + 7) / 8 packed bytes each
 * (pad bits ignored), as vsr_pair_distances: metric 4 / 5, the operator's float8.  dim 0 is valid here:
 * hamming_distance('', '') = 0, jaccard_distance('', '') = 1.  Unequal lengths: VSR_ERR_DIM_MISMATCH, "different bit lengths
 * %u and %u".  Host pointers. */
int vsr_bit_pair_distances(vsr_ctx* ctx, int metric, const uint8_t* a, const uint8_t* b, int64_t n_pairs,
                           int dim_a, int dim_b, int b_broadcast, double* out);
/* binary_quantize (vector.c:941-968) for n vectors: out[n][(dim + 7) / 8], bit i set where a[i] > 0 -- NaN, -0.0 and 0 give 0;
 * pad bits zero.  Host pointers. */
int vsr_binary_quantize(vsr_ctx* ctx, const float* a, int64_t n, int dim, uint8_t* out);
/* sparsevec's l2_distance / negative inner product / cosine_distance / l1_distance (sparsevec.c:803-1037) for n explicit pairs:
 * pair i is row i of the CSR triple a against row i of the CSR triple b (both validated as vsr_corpus_load_sparse validates rows).
 * One thread per pair runs pgvector's own sequential merge in pgvector's order, so out[i] is the operator's float8 bit for bit on
 * any data.  metric 0 .. 3.  dim_a != dim_b: VSR_ERR_DIM_MISMATCH, "different sparsevec dimensions %d and %d".  Host pointers. */
int vsr_sparse_pair_distances(vsr_ctx* ctx, int metric,
                              const int64_t* a_indptr, const int32_t* a_indices, const float* a_values,
                              const int64_t* b_indptr, const int32_t* b_indices, const float* b_values,
                              int64_t n_pairs, int dim_a, int dim_b, double* out);

/* ---- IVFFlat list probe (pgvector/src/ivfscan.c:36-176, 339-389) ------------------------------------------ */
/* An index = `lists` centres (lists x dim floats) and the list of every corpus row (row_list[n], caller row order): what
 * IVFFlat's build leaves in its list pages (ivfbuild.c, ivfkmeans.c).  The library keeps a list-ordered image of the rows
 * beside the corpus, so that a probe reads contiguous memory.  vsr_ivf_search = ivfflatgettuple's first call + the
 * executor's LIMIT and RLS filter: the `probes` nearest lists of each query (GetScanLists; equal centre distances: the
 * lower list first) are scanned exhaustively (GetScanItems) and the k nearest PERMITTED rows come back, same output
 * conventions as vsr_search.  Metric L2 / IP / COSINE as the opclasses define them (cosine: pass unit queries; the
 * centres are unit vectors; rows rank by negative inner product inside the lists and report the operator's value). */
typedef struct vsr_ivf vsr_ivf;
int vsr_ivf_load(vsr_corpus* corpus, const float* centers, int lists, const int32_t* row_list, vsr_ivf** out);
int vsr_ivf_free(vsr_ivf* ivf);       /* before vsr_corpus_free of its corpus */
/* index build, step 1 (ivfbuild.c:404-445 ComputeCenters -> ivfkmeans.c:21-93,259-498): k-means++ seeding and Elkan's
 * k-means over the sampled rows (samples[n_samples][dim], the caller samples max(lists * 50, 10000) rows like
 * ivfbuild.c:421-445); L2 for vector_l2_ops, the spherical variant for the inner-product and cosine opclasses.  The
 * random draws come from a seeded xorshift64* stream (PostgreSQL's RandomDouble is not reproducible outside a backend).
 * out_centers[lists][dim]; out_iterations (may be NULL) = Elkan iterations run.  Host pointers; synchronises. */
int vsr_ivf_kmeans(vsr_ctx* ctx, int metric, int dim, const float* samples, int64_t n_samples, int lists, uint64_t seed,
                   float* out_centers, int* out_iterations);
/* index build, step 2, the pass over every row (ivfbuild.c:141-227): out_row_list[i] = nearest of `lists` centres for caller
 * row i under the opclass distance, ties to the lower list id -- what vsr_ivf_load takes.  Host pointers; synchronises. */
int vsr_ivf_assign(vsr_corpus* corpus, const float* centers, int lists, int metric, int32_t* out_row_list);
int vsr_ivf_probe(vsr_ivf* ivf, const float* queries, int nq, int dim, int probes, int metric, int32_t* out_lists /* nq*probes */);
int vsr_ivf_search(vsr_ivf* ivf, const float* queries, int nq, int dim, int k, int probes, int metric,
                   const vsr_filter* const* filters,
                   int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts);
/* same with queries and results resident on the device (the serving form: nothing but the probed list ids, nq x probes x
 * 4 bytes, crosses PCIe, because the planner that groups queries by list is host code).  Returns when every query is
 * proven exact over its lists, like vsr_search_device_exact.  d_out_doc_ids / d_out_rows may be NULL. */
int vsr_ivf_search_device(vsr_ivf* ivf, const float* d_queries, int nq, int dim, int k, int probes, int metric,
                          const vsr_filter* const* filters,
                          int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                          int32_t* d_out_counts);
/* pgvector's iterative index scan for IVFFlat (ivfflat.iterative_scan = relaxed_order with ivfflat.max_probes: ivfscan.c:112-176
 * GetScanItems, :249-272, and the refill loop of ivfflatgettuple at :375-381; GUCs ivfflat.c:20-51).  Per query:
 *   1. List order.  P = min(probes, lists) and M = min(max(max_probes, probes), lists).  The M nearest centres are ordered
 *      nearest first, equal distances to the lower list id (GetScanLists with so->maxProbes), in the arithmetic of
 *      vsr_ivf_probe: the first P are exactly the lists vsr_ivf_probe(probes) returns.
 *   2. Batches.  Batch b holds lists b*P .. min((b+1)*P, M) - 1 of that order; the last batch may be short.  A batch's rows
 *      are ordered as vsr_ivf_search orders them: distance ascending, NaN last, then (document_id, block_id).
 *   3. Stream.  Batch 0, then batch 1, and so on; it is NOT re-sorted across batches ("relaxed order": a later batch may
 *      hold a nearer row).
 *   4. Filter and stop.  The query's filter decides which rows count; the answer is the first k permitted rows of the
 *      stream.  A batch is only begun while fewer than k have been found and lists remain; an empty batch does not stop the
 *      scan; fewer than k rows come back only when all M lists are exhausted.
 *   5. Prefix property.  The stream depends on neither k nor the filter's effect on the order: the answer for k1 is a
 *      prefix of the answer for k2 > k1 (a caller that ran dry asks again for more rows and skips what it already has).
 *   6. out_probes (may be NULL) = so->listIndex at the stop: the lists scanned, counted in whole batches.
 * mode: VSR_IVF_ITERATIVE_OFF is vsr_ivf_search bit for bit (max_probes is ignored, as pgvector ignores it; out_probes =
 * P); IVFFlat has no strict order; any other value is VSR_ERR_INVALID.  max_probes: 1 .. 32768 (the GUC's range), else
 * VSR_ERR_INVALID.  Metrics, k limits, the dimension message and the L1 refusal are vsr_ivf_search's.  Entries past the
 * count hold -1 / +Inf.  Batch 0 runs as vsr_ivf_search does; every later batch of every query runs in one further launch
 * with nothing crossing PCIe in between.  An index whose lists x dimensions x k do not fit the launch's 160 KiB of
 * on-chip memory (beyond ~2700 dimensions at 32768 lists) is VSR_ERR_UNSUPPORTED. */
typedef enum { VSR_IVF_ITERATIVE_OFF = 0, VSR_IVF_ITERATIVE_RELAXED = 1 } vsr_ivf_iterative;
int vsr_ivf_search_iterative(vsr_ivf* ivf, const float* queries, int nq, int dim, int k, int probes, int metric,
                             const vsr_filter* const* filters, int mode, int max_probes,
                             int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist,
                             int32_t* out_counts, int32_t* out_probes);
/* same with queries and results resident on the device, on vsr_ivf_search_device's contract: enqueued on the corpus
 * context's stream, returns when every query is proven exact.  d_out_doc_ids / d_out_rows / d_out_probes may be NULL. */
int vsr_ivf_search_iterative_device(vsr_ivf* ivf, const float* d_queries, int nq, int dim, int k, int probes, int metric,
                                    const vsr_filter* const* filters, int mode, int max_probes,
                                    int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                    int32_t* d_out_counts, int32_t* d_out_probes);

/* device memory of an index in bytes (the corpus: vsr_corpus_device_bytes).  Any index.  Counted: the list-ordered view's rows,
 * norms and rank map (and its screening planes where the fp32 corpus has them), the centres, the list offsets.  Not counted: what
 * is cached per filter (bitmaps in view order, per-list parts) and the lists' tile lists, as vsr_hnsw_device_bytes leaves out its
 * per-filter bitmaps. */
int64_t vsr_ivf_device_bytes(const vsr_ivf* ivf);

/* ---- IVFFlat over a halfvec corpus: halfvec_l2_ops / halfvec_ip_ops / halfvec_cosine_ops (ivfflat_halfvec_support, ivfutils.c:
 * 266-276, 305-314, 349-361; test/sql/ivfflat_halfvec.sql, test/t/032_ivfflat_halfvec_build_recall.pl) -----------------------------
 * vsr_ivf_kmeans_half, vsr_ivf_assign_half and vsr_ivf_load_half are vsr_ivf_kmeans, vsr_ivf_assign and vsr_ivf_load with every
 * float array -- samples, centres -- as binary16 bit patterns; vsr_ivf_load_half returns an index that EVERY float entry point above
 * takes: vsr_ivf_probe, vsr_ivf_search, vsr_ivf_search_device, vsr_ivf_search_iterative(_device), metric per call (L2, inner
 * product, cosine over unit rows rounded to binary16; L1: VSR_ERR_UNSUPPORTED, as for fp32 indexes).  The list-ordered image holds
 * the rows as the corpus does, 2 bytes per element, and the centres stay binary16 (K3h): no fp32 image of rows or centres exists on
 * the device, and vsr_ivf_device_bytes is about half that of the fp32 index over the widened rows (a quarter where that one
 * carries screening planes).
 *   - Centres are halfvec values.  A centre distance is the fp32 sum in element order, without contraction, of the widened centre
 *     against the query rounded to binary16 (Float4ToHalf, round to nearest even) and widened: what `$1::halfvec` computes
 *     (halfutils.c:27-40, 79-90).  Queries stay const float*; the probe and the iterative scan round as they load.  The assignment
 *     reads the corpus's binary16 rows where they lie.  Equal distances go to the lower list id.
 *   - Rows rank inside the lists exactly as vsr_search ranks a halfvec corpus.
 *   - k-means (vsr_ivf_kmeans_half): pgvector's for the type.  Sums and distances run in fp32 over the widened samples, and every
 *     value stored into a centre is rounded to binary16 (HalfvecUpdateCenter): the means, the random fill of an empty centre and of
 *     the no-sample case, the quotients of halfvec_l2_normalize (norm in double over the widened elements; overflow is looked for
 *     in the binary16 result).  Same seed and samples => the same centres as the float build with those roundings.
 *   - The host entry points refuse a finite query element that rounds to +-Inf (|v| >= 65520) with VSR_ERR_INVALID,
 *     `"<v>" is out of range for type halfvec`, as vsr_search does; the device entry points do not look.  A dimension mismatch is
 *     VSR_ERR_DIM_MISMATCH, "different halfvec dimensions %d and %d".
 *   - A corpus that is not a halfvec corpus: VSR_ERR_INVALID, "the corpus is not a halfvec corpus".  vsr_ivf_load / vsr_ivf_assign
 *     keep refusing a halfvec corpus (VSR_ERR_UNSUPPORTED, the message names the halfvec corpus and these entry points).
 *   - Everything else is the fp32 index's, unchanged: lists 1 .. 32768, probes, max_probes, the modes, the outputs, the prefix
 *     property, out_probes, filters, caller order against storage order, empty lists, n = 0, vsr_ivf_free.
 * The guarantee of the build is recall (032_ivfflat_halfvec_build_recall.pl's floors).  halfvec_l1_ops is not built. */
int vsr_ivf_load_half(vsr_corpus* half_corpus, const uint16_t* centers /* [lists][dim] binary16 bits */, int lists,
                      const int32_t* row_list, vsr_ivf** out);
int vsr_ivf_assign_half(vsr_corpus* half_corpus, const uint16_t* centers, int lists, int metric, int32_t* out_row_list);
int vsr_ivf_kmeans_half(vsr_ctx* ctx, int metric, int dim, const uint16_t* samples, int64_t n_samples, int lists, uint64_t seed,
                        uint16_t* out_centers, int* out_iterations);

/* ---- IVFFlat over a bit corpus: bit_hamming_ops (ivfflat_bit_support, ivfutils.c:248-252, 278-292, 316-323, 364-377;
 * test/sql/ivfflat_bit.sql, test/t/035_ivfflat_bit_build_recall.pl, test/t/036_ivfflat_bit_centers.pl) (K3b) ----------------------
 * The one ivfflat opclass of the type: list, row and k-means distance are all hamming_distance; there is no Jaccard opclass, no
 * norm procedure, nothing spherical.  dim counts bits, 1 .. 64000; lists 1 .. 32768.
 *   - Packed bit strings everywhere -- rows, queries, samples, centres: varbit order (vsr_corpus_load_bit's), ceil(dim / 8) bytes
 *     each; bits past dim in the last byte are ignored on every input, centres included, and clear on every output.
 *   - Centres are bit strings.  k-means (vsr_ivf_kmeans_bit) is pgvector's for the type: k-means++ and Elkan's bounds as in
 *     vsr_ivf_kmeans, the distance the Hamming count as a double; a new centre has bit i set where the fp32 quotient (members with
 *     bit i) / (members) > 0.5; an empty centre draws one value per bit from the serial stream, in (centre, bit) order, and takes
 *     the same > 0.5.  Every quantity is an integer or half-integer exact in fp32 and double, so the same seed and samples give the
 *     same centres and iteration count as a restatement on any host, bit for bit.  Samples and centres stay packed on the device.
 *   - Centre order: (Hamming count, list id), the lower list id first among equals -- one key for a (row or query, centre) pair in
 *     the probe, the assignment and the iterative scan.
 *   - Rows inside the lists rank as vsr_search_bit ranks them: ((float) Hamming count, document_id, block_id).
 *   - The list-ordered image holds the packed rows (16-byte chunks, as the corpus), their popcounts and the rank map; the centres
 *     stay packed: no fp32 image of anything.  The searches run K1b over the image: all filter modes, k <= VSR_MAX_K, the -1 / +Inf
 *     fill and vsr_stats_get as for vsr_search_bit; nothing is screened, nothing flags.
 *   - vsr_ivf_search_bit(_device) and vsr_ivf_search_bit_iterative(_device) have the contracts of vsr_ivf_search(_device) and
 *     vsr_ivf_search_iterative(_device) with packed queries; metric is VSR_METRIC_HAMMING.  vsr_ivf_free and vsr_ivf_device_bytes
 *     take the index as they take any.
 *   - Errors.  A corpus that is not a bit corpus: VSR_ERR_INVALID, "the corpus is not a bit corpus".  vsr_ivf_probe_bit /
 *     vsr_ivf_search_bit* on an index that is not over a bit corpus: VSR_ERR_INVALID, "the index is not over a bit corpus (it is
 *     searched with vsr_ivf_search*)".  vsr_ivf_probe, vsr_ivf_search* and vsr_ivf_search_iterative* on a bit index:
 *     VSR_ERR_UNSUPPORTED, "the index is over a bit corpus: it is searched with vsr_ivf_search_bit* (<~>)".  VSR_METRIC_JACCARD:
 *     VSR_ERR_UNSUPPORTED, "ivfflat has no bit_jaccard_ops operator class"; any other metric VSR_ERR_INVALID.  A dimension mismatch
 *     is VSR_ERR_DIM_MISMATCH, "different bit lengths %u and %u"; the format refusal wins over it.  probes, max_probes, mode, k,
 *     NULL and list-id checks are those of the float entry points. */
int vsr_ivf_kmeans_bit(vsr_ctx* ctx, int dim_bits, const uint8_t* samples /* [n][(dim+7)/8] */, int64_t n_samples, int lists,
                       uint64_t seed, uint8_t* out_centers /* [lists][(dim+7)/8] */, int* out_iterations);
int vsr_ivf_assign_bit(vsr_corpus* bit_corpus, const uint8_t* centers, int lists, int32_t* out_row_list);
int vsr_ivf_load_bit(vsr_corpus* bit_corpus, const uint8_t* centers, int lists, const int32_t* row_list, vsr_ivf** out);
int vsr_ivf_probe_bit(vsr_ivf* ivf, const uint8_t* queries, int nq, int dim, int probes, int32_t* out_lists /* nq*probes */);
int vsr_ivf_search_bit(vsr_ivf* ivf, const uint8_t* queries, int nq, int dim, int k, int probes, int metric,
                       const vsr_filter* const* filters,
                       int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts);
int vsr_ivf_search_bit_device(vsr_ivf* ivf, const uint8_t* d_queries, int nq, int dim, int k, int probes, int metric,
                              const vsr_filter* const* filters,
                              int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                              int32_t* d_out_counts);
int vsr_ivf_search_bit_iterative(vsr_ivf* ivf, const uint8_t* queries, int nq, int dim, int k, int probes, int metric,
                                 const vsr_filter* const* filters, int mode, int max_probes,
                                 int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist,
                                 int32_t* out_counts, int32_t* out_probes);
int vsr_ivf_search_bit_iterative_device(vsr_ivf* ivf, const uint8_t* d_queries, int nq, int dim, int k, int probes, int metric,
                                        const vsr_filter* const* filters, int mode, int max_probes,
                                        int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                        int32_t* d_out_counts, int32_t* d_out_probes);

/* ---- HNSW graph search (pgvector/src/hnswscan.c:15-45,179-316; hnswutils.c:813-976) -------------------------- */
/* A graph as pgvector's in-memory build leaves it (hnswbuild.c:357-470): n_elem elements, each with a top level, up to 10
 * heap TIDs (tids: caller row indices, -1 padded; identical vectors share an element), 2m neighbours on layer 0
 * (nbr0[n_elem][2m], -1 padded) and m per upper layer (up_nbr[n_upper][max_level][m] for the elements with level >= 1,
 * addressed through up_slot[n_elem]).  vsr_hnsw_search = hnswgettuple's first call + the executor's filter and LIMIT:
 * greedy descent (ef = 1) from `entry`, HnswSearchLayer with ef_search on layer 0, then the TIDs of the result elements
 * nearest first, the permission test per row and the first k.  Equal distances are ordered by element id.  Like the
 * reference with hnsw.iterative_scan = off, a filtered query can return fewer than k rows (vsr_hnsw_search_iterative below
 * runs pgvector's iterative scans).
 * out_visited (may be NULL): elements entered into the visited set by the layer-0 search, per query. */
typedef struct vsr_hnsw vsr_hnsw;
int vsr_hnsw_load(vsr_corpus* corpus, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                  const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                  int32_t n_upper, int32_t max_level, vsr_hnsw** out);
int vsr_hnsw_free(vsr_hnsw* index);   /* before vsr_corpus_free of its corpus */
int vsr_hnsw_search(vsr_hnsw* index, const float* queries, int nq, int dim, int k, int ef_search, int metric,
                    const vsr_filter* const* filters,
                    int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts,
                    int64_t* out_visited);

/* same, queries (nq x dim floats, row stride dim) and outputs in device memory, enqueued on the corpus context's stream in
 * ONE launch, no synchronisation.  On graphs beyond ~1M elements the visited set is a table in LDS sized by ef_search; a
 * query that outgrows it reports count -1 (never a partial result): vsr_hnsw_search re-runs such queries itself. */
/* index build (hnswbuild.c:357-470 in-memory build; hnswutils.c:1053-1346): batched insertion on the GPU over the corpus's rows
 * with m and ef_construction as the reloptions define them, levels from a seeded xorshift64* stream.  The
 * graph is not the serial build's graph -- neither is the reference's own parallel build's -- so against pgvector the
 * guarantee is recall (its test/t/012_hnsw_vector_build_recall.pl thresholds; tests/test_gpu_index.py).  The build itself is
 * deterministic: the same rows, seed, m, ef_construction and flags give the same graph, run to run -- the elements of a batch
 * search the graph as it stood when the batch began, candidates of equal distance are ordered by element id, and a
 * neighbour's reverse edges of one batch are applied in ascending source element.  On integer-valued rows (fp32 sums that do
 * not depend on their order) that graph is the one a serial restatement of the batched algorithm builds, array for array
 * (oracle/vsr_index_oracle.c: orc_hnsw_build_batched; tests/test_gpu_hnsw_build_model.py).
 * Never a thinner graph in silence: when a layer search fills its visited table (LDS, sized from m and ef_construction) the
 * build starts again with a table twice as large; VSR_ERR_UNSUPPORTED, naming ef_construction and m, when no larger one fits
 * or when reverse edges had to be dropped.  The session's guard word (vsr_screening_check) is left as it was found.
 * Identical vectors are not merged into one element (hnswbuild.c:329-351) by vsr_hnsw_build: every row is its own element
 * (vsr_hnsw_build_ex merges them).  Synchronises. */
int vsr_hnsw_build(vsr_corpus* corpus, int m, int ef_construction, int metric, uint64_t seed, vsr_hnsw** out);
/* vsr_hnsw_build with flags (unknown bits: VSR_ERR_INVALID).  flags = 0 is vsr_hnsw_build: the same graph for the same seed.
 * VSR_HNSW_BUILD_MERGE_DUPLICATES folds identical rows into one element carrying up to 10 heap TIDs, as pgvector does
 * (hnswbuild.c:309-355, called at :407).  ef_search bounds elements, not rows, so on a corpus with duplicates the merged graph
 * returns up to 10 x ef_search rows where the unmerged one returns at most ef_search.
 *   - Identical: the rows' dim fp32 values are byte-identical, on the rows as the corpus stores them (pgvector's
 *     datumIsEqual: +0.0 and -0.0 differ).
 *   - A group of g identical rows, in internal row order (the build's insertion order), becomes ceil(g / 10) elements.
 *     Element i of the group holds members 10i .. 10i + 9 in insertion order; its vector is its first member's row.
 *     Elements are numbered by their first member's position in insertion order.
 *   - The level stream is drawn once per row in insertion order (pgvector draws before its duplicate check); an element takes
 *     the level of its first row.  With the same seed, element e of the merged build is on the level the unmerged build
 *     gives row tids[e][0].
 *   - The grouping is exhaustive.  pgvector's is opportunistic (it compares a new element with its selected layer-0
 *     neighbours only): the serial build can miss a merge and splits groups of more than 10 differently, so TID lists are
 *     not comparable element by element; n_elem here <= n_elem there, and recall parity is the rest of the contract. */
#define VSR_HNSW_BUILD_MERGE_DUPLICATES 1u
int vsr_hnsw_build_ex(vsr_corpus* corpus, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out);
/* The graph of any index, loaded or built, as the arrays vsr_hnsw_load takes (vsr_hnsw_load of an export answers bit for bit
 * like the exported index).  vsr_hnsw_export_shape: what sizes them (any pointer may be NULL).  vsr_hnsw_export: host arrays
 * level[n_elem], nbr0[n_elem][2m], tid_count[n_elem], tids[n_elem][10] (caller row indices, -1 padded), up_slot[n_elem],
 * up_nbr[n_upper][max_level][m] (may be NULL when n_upper = 0).  Synchronises. */
int vsr_hnsw_export_shape(const vsr_hnsw* index, int32_t* m, int32_t* n_elem, int32_t* entry, int32_t* n_upper, int32_t* max_level);
int vsr_hnsw_export(const vsr_hnsw* index, int32_t* level, int32_t* nbr0, int32_t* tid_count, int64_t* tids, int32_t* up_slot,
                    int32_t* up_nbr);
int vsr_hnsw_info(const vsr_hnsw* index, int32_t* n_elem, int32_t* entry, int32_t* entry_level, int32_t* max_level);
/* INSERT into an indexed table (hnswinsert.c), for a batch of rows: extends a graph that exists instead of rebuilding it.  Takes
 * the arrays vsr_hnsw_load takes; the row format (fp32, halfvec or bit) comes from the corpus.
 *   - `corpus` holds the rows the prior graph was made over plus new rows.  The prior graph's heap TIDs are caller row indices
 *     of `corpus`, each covered row named once (n0 of them); that those rows ARE the vectors the graph was built on is the
 *     caller's contract and cannot be checked.
 *   - The new rows are the caller rows no TID names.  They are inserted in ascending internal row order, (document_id, block_id),
 *     the order vsr_hnsw_build inserts in: the i-th becomes element n_elem + i with that one TID.  Prior elements keep their ids,
 *     TID lists, levels and up_slot; new upper elements take slots n_upper, n_upper + 1, ... in element order; when a new element's
 *     level exceeds max_level the upper arrays are re-strided to the new max_level.
 *   - Levels: the seeded xorshift64* stream of vsr_hnsw_build, one draw per row; the i-th new row takes draw n0 + i.  Batches: the
 *     build's schedule max(1, min(done / 8, 4096, left)) with done starting at n_elem, its two phases, its entry-point rule, its
 *     visited-table restart (which begins again from the caller's arrays).  The per-edge distances the re-selection of a full list
 *     reads are not part of an export: they are recomputed from the rows on the GPU before the first batch.
 *     The schedule depends on done alone, so vsr_hnsw_build* of a prefix that ends at one of the full build's batch boundaries,
 *     extended over all rows with the build's seed, IS the full build's graph wherever that build is reproducible (integer-valued
 *     rows: tests/test_gpu_hnsw_extend.py compares array for array).  Off a boundary the graph is deterministic and a valid
 *     graph of the same batched algorithm, parity with pgvector being recall (test/t/013_hnsw_vector_insert_recall.pl's floors).
 *   - metric as for the matching build call: L2 / IP / cosine over unit rows (fp32, halfvec); Hamming / Jaccard over a bit
 *     corpus, where it is also the index's opclass.  m, ef_construction, halfvec dimension, a view corpus: the build's refusals.
 *   - flags must be 0: VSR_HNSW_BUILD_MERGE_DUPLICATES is VSR_ERR_UNSUPPORTED (an inserted row is never folded into an element,
 *     where pgvector would); a prior graph that HAS multi-TID elements is accepted and extended.
 *   - A sparse corpus: VSR_ERR_UNSUPPORTED, the message names sparsevec (the sparse build has no element -> row form).
 *   - The prior graph is written through, so it is checked on the host beyond vsr_hnsw_load's checks, VSR_ERR_INVALID naming the
 *     element: neighbour ids in [-1, n_elem); lists packed (no id after a -1); a neighbour on layer lc has level >= lc; up_slot in
 *     [0, n_upper) and distinct exactly where level >= 1, -1 elsewhere; entry on the highest level; no row under two TIDs.
 *   - n_elem = 0 (entry -1) is vsr_hnsw_build* with flags 0, the same graph; no new rows is vsr_hnsw_load*.
 * The result is an ordinary index (search, export, info, device_bytes, set_predicate_aware).  Synchronises. */
int vsr_hnsw_extend(vsr_corpus* corpus, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                    const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                    int32_t n_upper, int32_t max_level,
                    int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out);
/* VACUUM of an indexed table after DELETE (hnswvacuum.c): removes rows from a graph that exists, repairs every element that pointed
 * at a deleted one on the GPU and returns the compacted graph.  Takes the arrays vsr_hnsw_load takes, over the SAME corpus: the
 * deleted rows stay in it, because the repair walks through deleted elements and reads their vectors.  fp32, halfvec and bit corpora.
 *   - dead_rows[n_dead]: caller row indices.  A value outside [0, rows) is VSR_ERR_INVALID; duplicates are allowed; rows no heap TID
 *     names are ignored.  flags must be 0.
 *   - Pass 1 (host): the deleted TIDs leave their elements; an element lives while it has a TID left.  `highest` is the live element
 *     other than the entry with the greatest level, the lowest id among equals.
 *   - needs(e): a list of e names a deleted element, or e's layer-0 list is not full (NeedsUpdated).
 *   - Entry phase (RepairGraphEntryPoint), batches of one: highest is repaired from the entry, deleted or not, if needs(highest); a
 *     deleted entry is replaced by highest (none: the index is empty); a live entry is repaired from highest if needs(entry) (no
 *     highest: its lists become empty).
 *   - Main phase: every live e != entry with needs(e), ascending, computed ONCE after the entry phase, in batches of min(4096, left).
 *     pgvector re-evaluates NeedsUpdated as it goes; computing it once can only add repairs.
 *   - The repair of e is the build's search and selection against the graph as the batch found it, with beam ef_construction + 1:
 *     deleted elements and e itself are walked and stay in the working set, only live elements (e among them) count towards the beam,
 *     and both leave the candidates before the selection.  The batch's new lists are staged and installed together; the reverse
 *     edges are the build's records in the build's order, applied with UpdateNeighborOnDisk's cases: a source the list names already
 *     is skipped, a list that is not full takes it at its end, a full list gives up the first slot that names a deleted element,
 *     any other full list is re-selected (HnswUpdateConnection).
 *   - The result is compacted: live elements renumbered in ascending old id, upper slots in ascending old slot, max_level =
 *     max(1, level of the new entry) with the upper arrays at that stride, every list rewritten.  A live element keeps its surviving
 *     TIDs in their old order, moved to the front; its vector is the first survivor's row.  Everything deleted: the index
 *     vsr_hnsw_load makes of n_elem = 0, whose searches return count 0.
 *   - out_elem_map[n_elem] (may be NULL): the new id of every old element, -1 for a deleted one.  out_stats (may be NULL).
 *   - n_dead = 0 is vsr_hnsw_load* (a departure: pgvector would still repair lists that are not full).
 *   - Refusals: those of vsr_hnsw_extend -- a sparse corpus (VSR_ERR_UNSUPPORTED, the message names sparsevec), a view corpus, the
 *     build's limits on m, ef_construction, metric and halfvec dimension, and its host checks of the prior graph (written through).
 *   - A search that cannot find ef_construction live elements admits every candidate, so the working set of a mostly deleted graph
 *     outgrows the kernel's arrays in the LDS: the call then runs again with a visited table / candidate array twice as large,
 *     from the caller's arrays.  When nothing larger fits the LDS it runs once more in mixed form: the repairs that fit stay as
 *     they are, and each repair that does not is redone from scratch with its candidates (pgvector's two heaps), its selection
 *     scratch and an exact visited bitmap in a workspace in device memory, 28 bytes and one bit per element of the graph; a
 *     bounded pool of such workspaces is shared by the repairs that need one.  That form cannot overflow, so what is left to fail
 *     is the allocation of the pool (VSR_ERR_HIP).  The result depends neither on the initial sizes nor on which form a repair
 *     ran in.  Environment, read at every call: VSR_HNSW_VACUUM_SPILL=0 restores the refusal where the ladders end
 *     (VSR_ERR_UNSUPPORTED: rebuild over the live rows), =all runs every repair in the global-memory form; VSR_HNSW_VACUUM_LDS
 *     and VSR_HNSW_VACUUM_SPILL_WAVES bound the LDS the sizing believes in and the pool.
 * To drop the deleted rows from the corpus too: export the result, remap its TIDs, load a corpus without them and vsr_hnsw_load.
 * UPDATE is vacuum followed by vsr_hnsw_extend.  The result is an ordinary index.  Synchronises. */
typedef struct {
    int64_t tuples_removed, tuples_kept;   /* heap TIDs deleted / left */
    int32_t elements_removed;              /* elements whose last TID went */
    int32_t elements_repaired;             /* repairs run (entry phase included) */
    int32_t batches;                       /* repair batches of the attempt that succeeded (entry phase included) */
    int32_t attempts;                      /* 1 + restarts with larger arrays; 0: nothing ran on the GPU */
} vsr_hnsw_vacuum_stats;
int vsr_hnsw_vacuum(vsr_corpus* corpus, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                    const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                    int32_t n_upper, int32_t max_level, int ef_construction, int metric,
                    const int64_t* dead_rows, int64_t n_dead, uint32_t flags,
                    int32_t* out_elem_map /* [n_elem] new id or -1, may be NULL */, vsr_hnsw_vacuum_stats* out_stats /* may be NULL */,
                    vsr_hnsw** out);
/* The HNSW graphs of many row subsets of one corpus -- one index per role table or per dynamic partition -- built in ONE call, the
 * vectors resident once.  The row format (fp32, halfvec or bit) comes from the corpus, as for vsr_hnsw_extend.
 *   - Partition g is the caller rows part_rows[part_off[g] .. part_off[g + 1]); part_off[n_parts + 1] ascends from part_off[0] = 0.
 *     Partitions may overlap each other (a document can belong to several roles), come in any order and be empty.  Within ONE
 *     partition a row named twice, or a row outside [0, rows), is VSR_ERR_INVALID, the message naming the partition and the position.
 *   - out[g] is an ordinary index over `corpus` (search, iterative search, predicate-aware walk, export, info, device_bytes) that
 *     owns its arrays.  Its export equals, array for array, the export of vsr_hnsw_build / _half / _bit(m, ef_construction, metric,
 *     seed) over a corpus holding only partition g's rows with their (document_id, block_id), the heap TIDs mapped through
 *     part_rows: element e is the e-th row of the partition in internal (document_id, block_id) order; the level stream starts afresh
 *     from `seed` for every partition; every partition follows the build's schedule from done = 0 and the build's entry-point rule;
 *     every graph has its own max_level and its own upper-slot numbering.  An empty partition gives the index vsr_hnsw_load makes of
 *     n_elem = 0.  n_parts = 0 succeeds and writes nothing.
 *   - How: all partitions are built in one global element space by the build's kernels; a round serves the next batch of every
 *     partition that has one due while the round's elements stay within 4096 (one search launch, one sort and one link launch per
 *     round, where building the graphs one after the other takes those per batch and partition), and one last launch writes every
 *     graph's own arrays.  The packing into rounds does not change any graph.  VSR_HNSW_FOREST_BATCH=<1..4096> (read at every call;
 *     anything else: VSR_ERR_INVALID) lowers the cap, so that waiting can be exercised on small inputs; a batch larger than the cap
 *     takes a round of its own.  A visited-table overflow in any graph restarts the whole call with twice the slots
 *     (VSR_HNSW_BUILD_VISITED_SLOTS applies); dropped records are the build's refusal.
 *   - metric, m, ef_construction, halfvec dimension, a view corpus: the rules and refusals of the matching build call.  A sparse
 *     corpus: VSR_ERR_UNSUPPORTED, the message names sparsevec (the sparse build has no element -> row form).  flags must be 0:
 *     VSR_HNSW_BUILD_MERGE_DUPLICATES is VSR_ERR_UNSUPPORTED, any other bit VSR_ERR_INVALID.
 *   - On failure every index made so far is freed and every out[g] is NULL.  The session's guard word is left as it was found.
 * Not covered: vacuuming a partition graph in place (export it and use vsr_hnsw_vacuum).  New rows go into many partition graphs with
 * vsr_hnsw_extend_partitions below.  The graphs of a query's partitions are searched as a set by vsr_hnsw_forest_search*.  Synchronises. */
int vsr_hnsw_build_partitions(vsr_corpus* corpus, int n_parts,
                              const int64_t* part_off  /* [n_parts + 1], ascending, part_off[0] = 0 */,
                              const int64_t* part_rows /* [part_off[n_parts]] caller row indices */,
                              int m, int ef_construction, int metric, uint64_t seed, uint32_t flags,
                              vsr_hnsw** out /* [n_parts] */);
/* vsr_hnsw_extend for many graphs over ONE resident corpus in one call: partition g's graph prior[g] takes the caller rows
 * new_rows[new_off[g] .. new_off[g + 1]) -- a role was granted documents, new documents arrived -- and out[g] is the new index.
 *   - prior[g] is any index over `corpus` (from vsr_hnsw_build_partitions, from this call, from vsr_hnsw_load*, ...); NULL or an index of
 *     n_elem = 0 is the empty graph.  Two partitions may name one prior index.  The priors are read on the device, are not modified and
 *     stay the caller's.  All priors share one m, which the call takes from them: when every prior[g] is NULL, m is not known and the
 *     call is refused with VSR_ERR_INVALID (such graphs are vsr_hnsw_build_partitions').
 *   - Partitions may share rows; within ONE partition a row named twice, or a row outside [0, rows), is VSR_ERR_INVALID naming the
 *     partition and the position, and a new row that the prior graph already holds under a heap TID is VSR_ERR_INVALID naming the
 *     partition and the row.
 *   - out[g] is, array for array in its export, what vsr_hnsw_extend(ef_construction, metric, seed) makes of export(prior[g]) over a
 *     corpus that holds only graph g's rows, old and new, with their (document_id, block_id), TIDs mapped there and back: prior
 *     elements keep ids, TID lists, levels and upper slots; the new rows become elements n_elem + i in ascending internal
 *     (document_id, block_id) order with one TID each; the i-th takes level draw n0 + i, n0 being the prior's heap TIDs; batches are the
 *     build's from done = n_elem, with the build's entry-point rule; new upper slots continue after the prior ones and the upper
 *     arrays are re-strided when the top level rises.  So priors that are vsr_hnsw_build_partitions graphs of prefixes ending at batch
 *     boundaries, extended with the build's seed, give the graphs vsr_hnsw_build_partitions makes of the full partitions.
 *     A partition without new rows gets an index whose export equals its prior's.  n_parts = 0 succeeds and writes nothing.
 *   - How: the graphs that take rows are joined on the device into the global element space of vsr_hnsw_build_partitions, the prior
 *     edges' distances are recomputed there, and the rounds, VSR_HNSW_FOREST_BATCH, VSR_HNSW_BUILD_VISITED_SLOTS and the restart (from
 *     the priors, with twice the visited slots) are that call's.
 *   - An index this library made (build, build_partitions, extend, extend_partitions, vacuum) is written through as it is.  Any other
 *     prior that takes rows is first brought to the host and put through vsr_hnsw_extend's checks; a failure is VSR_ERR_INVALID naming
 *     the partition, and nothing is launched.  The result of a partition WITHOUT new rows is a plain copy that nobody read: it counts as
 *     made by this library only if its prior did, so the copy of a loaded index is checked like the loaded index when a later call gives
 *     it rows.
 *   - metric, ef_construction against m, halfvec dimension, a view corpus: the rules and refusals of vsr_hnsw_extend; on a bit corpus
 *     metric must be the priors' opclass.  A sparse corpus: VSR_ERR_UNSUPPORTED, the message names sparsevec.  flags must be 0:
 *     VSR_HNSW_BUILD_MERGE_DUPLICATES is VSR_ERR_UNSUPPORTED, any other bit VSR_ERR_INVALID.  A prior over another corpus, of another
 *     row format, m or bit opclass: VSR_ERR_INVALID naming the partition.
 *   - On failure every index made so far is freed and every out[g] is NULL.  The session's guard word is left as it was found.
 * Not covered: vacuuming many partitions in one call, changing a prior in place, appending rows to the resident corpus.  Synchronises. */
int vsr_hnsw_extend_partitions(vsr_corpus* corpus, int n_parts,
                               vsr_hnsw* const* prior   /* [n_parts], an entry may be NULL */,
                               const int64_t* new_off   /* [n_parts + 1], ascending from 0 */,
                               const int64_t* new_rows  /* [new_off[n_parts]] caller row indices */,
                               int ef_construction, int metric, uint64_t seed, uint32_t flags,
                               vsr_hnsw** out           /* [n_parts] */);
/* A FOREST: many indexes over ONE corpus (the graphs of vsr_hnsw_build_partitions, or any others) searched as a set -- what the
 * reference's dynamic_partition_search does with the HNSW indexes of a user's role combination: search each, merge by distance, drop the
 * rows several partitions hold, keep k.  Here: ONE search launch over all (query, graph) pairs of the call and ONE merge launch.
 *   - vsr_hnsw_forest_open validates once: every index over the same corpus, of the same row format (fp32, halfvec or bit) and the same m,
 *     bit indexes of the same opclass; a sparse index is VSR_ERR_UNSUPPORTED (the message names sparsevec), anything else
 *     VSR_ERR_INVALID, the message naming the offending index.  n_indexes = 0 and empty graphs are allowed; an index may be named
 *     twice.  The forest uploads one descriptor per graph and owns the scratch of its calls; the indexes stay the caller's and must
 *     outlive the forest: vsr_hnsw_forest_free comes before vsr_hnsw_free of its indexes.
 *   - A TASK is a (query, graph) pair: query i owns tasks q_off[i] .. q_off[i + 1] of q_graph (graph ids are positions in `indexes`).
 *     q_off must be non-decreasing from 0 and every graph id within range (checked on the host: VSR_ERR_INVALID).  A query may have no
 *     task (its count is 0) and may name a graph twice.
 *   - The result of query i: the rows vsr_hnsw_search / vsr_hnsw_search_bit returns for that query, filter, k, ef_search and metric on
 *     each of its graphs, put together, ordered by (the index's rank value, document_id, block_id), repeated rows dropped, the first k
 *     kept.  Distances are reported as vsr_hnsw_search reports them; slots past the count hold -1 / +Inf.  filters: as vsr_hnsw_search,
 *     one per QUERY (or NULL).  Predicate-aware walking is a property of the forest on this path (vsr_hnsw_forest_set_predicate_aware,
 *     off by default); the indexes' own flags are not read.
 *   - out_visited, [q_off[nq]], may be NULL: per TASK, what vsr_hnsw_search reports per query.
 *   - A task whose LDS visited table overflows has no result.  The device forms then report count -1 for its query, never a partial
 *     result; the host forms run exactly those tasks again with the global bitmap and merge again.  VSR_HNSW_VISITED applies as in
 *     vsr_hnsw_search.
 *   - The device forms take d_queries and the outputs in device memory, q_off / q_graph / filters in host memory, and enqueue on the
 *     corpus context's stream: the task table's upload, (bit: one staging launch over the queries,) the search launch, the merge launch.
 *     They wait only where vsr_hnsw_search_device does: for the previous call's pinned upload blocks.  Over an empty forest only
 *     nq = 0 is answered (there is no context to enqueue on); the host forms answer count 0.
 *   - VSR_HNSW_FOREST_MERGE_KEYS=<C> (read at every call): the key slots of the merge's LDS, a power of two from the smallest one
 *     >= 2 k to 16384, anything else VSR_ERR_INVALID; default 2048, or the lower bound when that is larger.  It sets how many task lists
 *     one merge pass takes and never changes a result.
 * Out of scope: iterative scans over a forest, forests of sparse indexes, and forests that span GPUs. */
typedef struct vsr_hnsw_forest vsr_hnsw_forest;
int vsr_hnsw_forest_open(vsr_hnsw* const* indexes, int n_indexes, vsr_hnsw_forest** out);
int vsr_hnsw_forest_free(vsr_hnsw_forest* forest);
int vsr_hnsw_forest_set_predicate_aware(vsr_hnsw_forest* forest, int on);
int vsr_hnsw_forest_search(vsr_hnsw_forest* forest, const float* queries, int nq, int dim, int k, int ef_search, int metric,
                           const int64_t* q_off /* [nq + 1] */, const int32_t* q_graph /* [q_off[nq]] */,
                           const vsr_filter* const* filters /* [nq] or NULL */,
                           int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts,
                           int64_t* out_visited /* [q_off[nq]], per task, may be NULL */);
int vsr_hnsw_forest_search_device(vsr_hnsw_forest* forest, const float* d_queries, int nq, int dim, int k, int ef_search, int metric,
                                  const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters,
                                  int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                  int32_t* d_out_counts, int64_t* d_out_visited);
/* ... over a forest of bit indexes: queries are packed bit strings of (dim + 7) / 8 bytes, metric the indexes' opclass */
int vsr_hnsw_forest_search_bit(vsr_hnsw_forest* forest, const uint8_t* queries, int nq, int dim, int k, int ef_search, int metric,
                               const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters,
                               int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts,
                               int64_t* out_visited);
int vsr_hnsw_forest_search_bit_device(vsr_hnsw_forest* forest, const uint8_t* d_queries, int nq, int dim, int k, int ef_search, int metric,
                                      const int64_t* q_off, const int32_t* q_graph, const vsr_filter* const* filters,
                                      int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                      int32_t* d_out_counts, int64_t* d_out_visited);
/* What the vacuum that made this index spilled: repairs run in the global-memory form, and the bytes of the workspace pool.
 * 0 / 0 for an index any other call made. */
int vsr_hnsw_vacuum_spill_info(const vsr_hnsw* index, int32_t* spilled_repairs, int64_t* workspace_bytes);
/* Predicate-aware walk (off by default: pgvector filters what the index returns, hnswscan.c + the executor's RLS qual).  On:
 * the layer-0 search of later vsr_hnsw_search* calls applies the query's filter while it walks, ACORN-1 style -- the result
 * set and the candidate set hold permitted elements only, and an expansion also takes the permitted neighbours of its
 * neighbours that are not permitted -- which is what acorn_benchmark/src/acorn_search.cpp:144-181 gets from the ACORN
 * library (its source is not part of the reference tree: parity is with the index oracle's restatement of this walk and
 * with the exact filtered scan by recall).  Queries without a filter are searched as before. */
int vsr_hnsw_set_predicate_aware(vsr_hnsw* index, int on);
int vsr_hnsw_search_device(vsr_hnsw* index, const float* d_queries, int nq, int dim, int k, int ef_search, int metric,
                           const vsr_filter* const* filters,
                           int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                           int32_t* d_out_counts, int64_t* d_out_visited);

/* Iterative index scans: hnsw.iterative_scan = relaxed_order | strict_order with hnsw.max_scan_tuples (hnswscan.c:47-76,
 * 227-312; hnswutils.c:813-976; GUCs hnsw.c:21-31,90-102), i.e. hnswgettuple called until the executor's LIMIT is met.
 * Per query: a visited set V that lasts the whole scan, a discarded set D ordered by (index distance, element id), a
 * counter T (so->tuples) and P = -inf (so->previousDistance).
 *   1. Round 0 is vsr_hnsw_search's walk.  T counts the layer-0 entry point plus the unvisited neighbours of every
 *      expansion (= out_visited).  D receives every neighbour that fails admission and every element pushed out of W.
 *   2. Emission: W nearest first, each element's heap TIDs newest first.  strict_order drops a TID whose element's index
 *      distance is below P, else P takes that distance.  A TID the query's filter admits is a result; k results stop it.
 *   3. W exhausted: if T >= max_scan_tuples, D's smallest element is the next W alone (stop when D is empty); otherwise
 *      stop when D is empty, else the min(ef_search, |D|) smallest elements leave D and are the entry points of another
 *      layer-0 search with ef_search (not marked or counted again; T grows by the unvisited neighbours of expansions, both
 *      kinds of discard go to D again), whose W is the next batch.
 *   4. Not modelled: pgvector's memory stop (work_mem x hnsw.scan_mem_multiplier): only max_scan_tuples ends the search.
 * Rows come back in stream order, not re-sorted (relaxed_order can be out of order, as in pgvector).  The stream depends
 * on neither k nor the filter, which only decide where it stops: the answer for k1 is a prefix of the answer for k2 > k1.
 * mode VSR_HNSW_ITERATIVE_OFF is vsr_hnsw_search bit for bit (out_tuples = out_visited).  max_scan_tuples: 1 .. INT_MAX;
 * anything else, or an unknown mode: VSR_ERR_INVALID.  A mode other than off on a predicate-aware index:
 * VSR_ERR_UNSUPPORTED.  out_tuples (may be NULL): T when the query's scan stopped.  D lives in device memory with room
 * for max_scan_tuples plus one round; a query that outgrows it is re-run by the host entry point with room for every
 * element.  The _device variant (device pointers, one launch per chunk of queries on the corpus context's stream, no
 * synchronisation) reports such a query with count -1 instead. */
typedef enum {
    VSR_HNSW_ITERATIVE_OFF = 0,
    VSR_HNSW_ITERATIVE_RELAXED = 1,
    VSR_HNSW_ITERATIVE_STRICT = 2
} vsr_hnsw_iterative;
int vsr_hnsw_search_iterative(vsr_hnsw* index, const float* queries, int nq, int dim, int k, int ef_search, int metric,
                              const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                              int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist,
                              int32_t* out_counts, int64_t* out_tuples);
int vsr_hnsw_search_iterative_device(vsr_hnsw* index, const float* d_queries, int nq, int dim, int k, int ef_search, int metric,
                                     const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                                     int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                     int32_t* d_out_counts, int64_t* d_out_tuples);

/* device memory of an index's graph arrays, in bytes (the corpus: vsr_corpus_device_bytes).  Any index; the row format of the
 * corpus does not enter, so an index over halfvec rows and one over their fp32 image loaded from the same arrays agree. */
int64_t vsr_hnsw_device_bytes(const vsr_hnsw* index);

/* ---- HNSW over a halfvec corpus: halfvec_l2_ops / halfvec_ip_ops / halfvec_cosine_ops (hnsw_halfvec_support,
 * hnswutils.c:1385-1396; test/sql/hnsw_halfvec.sql, test/t/024_hnsw_halfvec_build_recall.pl) ------------------------------------
 * vsr_hnsw_load_half takes the arrays of vsr_hnsw_load, vsr_hnsw_build_half the arguments of vsr_hnsw_build_ex; both return an
 * index that EVERY float search entry point above takes: vsr_hnsw_search, vsr_hnsw_search_device,
 * vsr_hnsw_search_iterative(_device), metric per call (L2, inner product, cosine over unit rows rounded to binary16; L1:
 * VSR_ERR_UNSUPPORTED, as for fp32 graphs).  The graph kernels gather the binary16 rows themselves (K4h): no fp32 image of the
 * rows is made anywhere, and vsr_hnsw_device_bytes equals that of an fp32 index loaded from the same arrays.
 *   - Arithmetic: pgvector's for the type (halfutils.c) -- both operands widened to fp32, fp32 sums.  Queries stay
 *     const float*; the search kernel rounds every query element to binary16 (Float4ToHalf, round to nearest even) as it loads
 *     the query.  There is no staging launch: vsr_hnsw_search_device stays ONE launch, the iterative form one per chunk of queries.
 *   - Reported distances follow vsr_hnsw_search's rule for fp32 indexes.
 *   - The host entry points refuse a finite query element that rounds to +-Inf (|v| >= 65520) with VSR_ERR_INVALID,
 *     `"<v>" is out of range for type halfvec`, as vsr_search does; the device entry points do not look.  A dimension mismatch is
 *     VSR_ERR_DIM_MISMATCH, "different halfvec dimensions %d and %d".
 *   - A corpus that is not a halfvec corpus: VSR_ERR_INVALID.  More than 4000 dimensions (HNSW_MAX_DIM * 2, hnswutils.c:1390):
 *     VSR_ERR_UNSUPPORTED, "column cannot have more than 4000 dimensions for hnsw index".  m, ef_construction, flags and metrics
 *     are checked exactly as vsr_hnsw_build_ex checks them.
 *   - vsr_hnsw_load / vsr_hnsw_build / vsr_hnsw_build_ex keep refusing a halfvec corpus (VSR_ERR_UNSUPPORTED, the message names
 *     the halfvec corpus and these entry points).  vsr_hnsw_search_bit* on a half index: VSR_ERR_INVALID, as on any non-bit index.
 *   - Everything else is vsr_hnsw_search's, unchanged: vsr_hnsw_set_predicate_aware, the iterative modes, the visited-set forms
 *     and both re-runs, vsr_hnsw_export*, vsr_hnsw_info, vsr_hnsw_free, filters, row_offset, up to 10 TIDs per element.
 * The merging build (VSR_HNSW_BUILD_MERGE_DUPLICATES) keeps vsr_hnsw_build_ex's grouping contract; identical means the binary16
 * bytes are identical, so +0.0 and -0.0 differ: datumIsEqual on a halfvec.  The guarantee is recall, as for the float build
 * (024_hnsw_halfvec_build_recall.pl's floor, 0.98 for all three opclasses).  halfvec_l1_ops is not built. */
int vsr_hnsw_load_half(vsr_corpus* half_corpus, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                       const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                       int32_t n_upper, int32_t max_level, vsr_hnsw** out);
int vsr_hnsw_build_half(vsr_corpus* half_corpus, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out);

/* ---- HNSW over a bit corpus: bit_hamming_ops / bit_jaccard_ops (hnsw_bit_support, hnswutils.c:1398-1410; test/sql/hnsw_bit.sql,
 * test/t/020_hnsw_bit_build_recall.pl, 023_hnsw_bit_duplicates.pl) --------------------------------------------------------------
 * An HNSW index belongs to one opclass: the graph is built for one distance, so `metric` (VSR_METRIC_HAMMING or
 * VSR_METRIC_JACCARD) is fixed when the index is made, by vsr_hnsw_load_bit (the arrays of vsr_hnsw_load) or vsr_hnsw_build_bit.
 * vsr_hnsw_load / vsr_hnsw_build* keep refusing a bit corpus (VSR_ERR_UNSUPPORTED, the message names the bit corpus and these
 * entry points); these refuse a corpus that is not a bit corpus and a metric other than 4 / 5 with VSR_ERR_INVALID.
 *   - Queries: (dim + 7) / 8 packed bytes each, varbit order; device queries need no alignment.  Bits past dim are ignored:
 *     staging clears them, as vsr_search_bit's does.
 *   - dim must be the corpus's bit length, else VSR_ERR_DIM_MISMATCH, "different bit lengths %u and %u", the column's first
 *     (CheckDims, bitvec.c:32-39).
 *   - metric must be the index's; a mismatch is VSR_ERR_INVALID naming both.  It catches misuse, it selects nothing.
 *   - The float vsr_hnsw_search* on a bit index: VSR_ERR_UNSUPPORTED, the message names the bit corpus.  vsr_hnsw_search_bit* on
 *     an index over any other corpus: VSR_ERR_INVALID.
 *   - Index distance: Hamming is the integer count, exact in fp32; Jaccard is evaluated in double as bitutils.c:96-129 does (no
 *     common bit: 1) and rounded to fp32, exactly the value vsr_search_bit reports.  Candidate keys are monotone(fp32) << 32 |
 *     element id as in vsr_hnsw_search: equal distances -- the rule among Hamming distances -- are ordered by element id.
 *     out_dist is that fp32 value (no square root).
 *   - Everything else is vsr_hnsw_search's, unchanged: vsr_hnsw_set_predicate_aware, the iterative modes (relaxed, strict,
 *     max_scan_tuples, the re-run of a query whose discarded set overflowed), the visited-set forms and the re-run of a query
 *     whose LDS table overflowed (the device entry points report it with count -1), vsr_hnsw_export*, vsr_hnsw_info,
 *     vsr_hnsw_free, the filters of the bit corpus, row_offset, up to 10 TIDs per element, m 2 .. 100, ef_search 1 .. 5000.
 *   - The device entry points enqueue the query staging and ONE search launch (iterative: one per chunk of queries) on the
 *     corpus context's stream and do not synchronise.
 * vsr_hnsw_build_bit is vsr_hnsw_build_ex over bit rows: the same batched insertion, the same seeded level stream, flags 0 or
 * VSR_HNSW_BUILD_MERGE_DUPLICATES with exactly the grouping contract written there.  Identical means the packed bytes are
 * identical; pad bits are zero on load, so this is datumIsEqual on a bit(n).  Quantized corpora are full of duplicates: the
 * merging build is the one to use.  The guarantee is recall, as for the float build (020_hnsw_bit_build_recall.pl's floors). */
int vsr_hnsw_load_bit(vsr_corpus* bits, int metric, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                      const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                      int32_t n_upper, int32_t max_level, vsr_hnsw** out);
int vsr_hnsw_build_bit(vsr_corpus* bits, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out);
int vsr_hnsw_search_bit(vsr_hnsw* index, const uint8_t* queries, int nq, int dim, int k, int ef_search, int metric,
                        const vsr_filter* const* filters,
                        int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts,
                        int64_t* out_visited);
int vsr_hnsw_search_bit_device(vsr_hnsw* index, const uint8_t* d_queries, int nq, int dim, int k, int ef_search, int metric,
                               const vsr_filter* const* filters,
                               int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                               int32_t* d_out_counts, int64_t* d_out_visited);
int vsr_hnsw_search_bit_iterative(vsr_hnsw* index, const uint8_t* queries, int nq, int dim, int k, int ef_search, int metric,
                                  const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                                  int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist,
                                  int32_t* out_counts, int64_t* out_tuples);
int vsr_hnsw_search_bit_iterative_device(vsr_hnsw* index, const uint8_t* d_queries, int nq, int dim, int k, int ef_search, int metric,
                                         const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                                         int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                         int32_t* d_out_counts, int64_t* d_out_tuples);
/* K4s -- HNSW over a sparse corpus (vsr_corpus_load_sparse): pgvector's sparsevec_l2_ops / sparsevec_ip_ops /
 * sparsevec_cosine_ops / sparsevec_l1_ops (hnswutils.c:1352-1361, 1411-1422), the type's whole index story (it has no IVFFlat
 * opclass).  vsr_hnsw_load_sparse takes the arrays of vsr_hnsw_load, vsr_hnsw_build_sparse the arguments of vsr_hnsw_build_ex with
 * metric VSR_METRIC_L2 .. VSR_METRIC_L1; the metric of a search is given per call, as for the float indexes, L1 included.  Cosine
 * follows K4's convention: the caller loads unit rows (vsr_sparse_l2_normalize) and passes unit queries.
 *   - Refusals of load and build: a corpus that is not sparse, VSR_ERR_INVALID "<entry point>: the corpus is not a sparse corpus";
 *     a corpus with a row of more than 1000 non-zeros (HNSW_MAX_NNZ, checkValue of the opclasses), VSR_ERR_UNSUPPORTED
 *     "sparsevec cannot have more than 1000 non-zero elements for hnsw index"; VSR_HNSW_BUILD_MERGE_DUPLICATES,
 *     VSR_ERR_UNSUPPORTED (the pre-pass compares fixed-stride rows).  m, ef_construction, seed: vsr_hnsw_build_ex's rules.
 *   - Queries are CSR, as vsr_search_sparse takes them and validated as it validates them (host forms); pgvector checks only
 *     indexed values, so a query may carry up to 16000 non-zeros.  The _device forms take the three arrays in device memory and
 *     max_query_nnz, which sizes the staged tables: a longer (or malformed) query becomes an empty table and sets bit value 8 of the
 *     guard word (vsr_screening_check), exactly as in vsr_search_sparse_device.  Query staging and the search are launches on the
 *     corpus context's stream with no host round trip.
 *   - Index distance: squared L2, the L1 sum, the negated inner product (inner product and cosine opclasses); ties by element id.
 *     Reported distances: vsr_hnsw_search's rule, and <+> reports the sum itself.  Arithmetic is vsr_search_sparse's: fp32 over
 *     a row's entries, the query entries no row entry meets as (float) of a double difference.
 *   - The float and bit search entry points on a sparse index: VSR_ERR_UNSUPPORTED, the message names these entry points; these
 *     entry points on another index: VSR_ERR_INVALID.
 *   - Everything else is vsr_hnsw_search's, unchanged: vsr_hnsw_set_predicate_aware, the iterative modes with max_scan_tuples, the
 *     visited-set forms and both re-runs, vsr_hnsw_export*, vsr_hnsw_info, vsr_hnsw_device_bytes, vsr_hnsw_free, filters, row_offset,
 *     up to 10 TIDs per element. */
int vsr_hnsw_load_sparse(vsr_corpus* sparse_corpus, int m, int32_t n_elem, int32_t entry, const int32_t* level, const int32_t* nbr0,
                         const int32_t* tid_count, const int64_t* tids, const int32_t* up_slot, const int32_t* up_nbr,
                         int32_t n_upper, int32_t max_level, vsr_hnsw** out);
int vsr_hnsw_build_sparse(vsr_corpus* sparse_corpus, int m, int ef_construction, int metric, uint64_t seed, uint32_t flags, vsr_hnsw** out);
int vsr_hnsw_search_sparse(vsr_hnsw* index, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq, int dim,
                           int k, int ef_search, int metric, const vsr_filter* const* filters,
                           int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts,
                           int64_t* out_visited);
int vsr_hnsw_search_sparse_device(vsr_hnsw* index, const int64_t* d_q_indptr, const int32_t* d_q_indices, const float* d_q_values,
                                  int nq, int dim, int max_query_nnz, int k, int ef_search, int metric,
                                  const vsr_filter* const* filters,
                                  int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                  int32_t* d_out_counts, int64_t* d_out_visited);
int vsr_hnsw_search_sparse_iterative(vsr_hnsw* index, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq,
                                     int dim, int k, int ef_search, int metric, const vsr_filter* const* filters, int mode,
                                     int64_t max_scan_tuples,
                                     int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist,
                                     int32_t* out_counts, int64_t* out_tuples);
int vsr_hnsw_search_sparse_iterative_device(vsr_hnsw* index, const int64_t* d_q_indptr, const int32_t* d_q_indices,
                                            const float* d_q_values, int nq, int dim, int max_query_nnz, int k, int ef_search,
                                            int metric, const vsr_filter* const* filters, int mode, int64_t max_scan_tuples,
                                            int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                            int32_t* d_out_counts, int64_t* d_out_tuples);
/* The two vector functions the cosine opclass needs, for n sparse vectors at once (host pointers; only the offsets and the values
 * enter): sparsevec_l2_norm (sparsevec.c:1044-1055: a double sum of double products, then sqrt) and sparsevec_l2_normalize
 * (sparsevec.c:1060-1120: (float) (v / norm) per entry with the norm in double; a zero norm leaves the row as it is; an infinite
 * result fails with "value out of range: overflow").  out_values has one value per input entry; *out_zeros (may be NULL) counts
 * the entries that became 0 -- the caller drops them, as pgvector does, so that the result is a legal sparsevec. */
int vsr_sparse_norms(vsr_ctx* ctx, const int64_t* indptr, const float* values, int64_t n, double* out);
int vsr_sparse_l2_normalize(vsr_ctx* ctx, const int64_t* indptr, const float* values, int64_t n, float* out_values, int64_t* out_zeros);

/* The indexed two-stage search -- pgvector's documented use of binary_quantize: CREATE INDEX ... USING hnsw
 * ((binary_quantize(embedding)::bit(n)) bit_hamming_ops), ORDER BY ... <~> ... LIMIT shortlist, then the re-rank on the original
 * vectors.  It is vsr_search_quantized with stage 1 replaced by the index: qb = binary_quantize(q); S = the answer of
 * vsr_hnsw_search_bit(bit_index, qb, k = shortlist, ef_search, VSR_METRIC_HAMMING, filters), which may hold fewer than
 * `shortlist` rows, as any HNSW scan may; stage 2 is vsr_search_quantized's exact re-rank on `source`, unchanged.  bit_index must
 * be a Hamming index over the corpus vsr_corpus_binary_quantize(source) made, else VSR_ERR_INVALID in vsr_search_quantized's
 * words.  Plain walk or predicate-aware as the index is set; no iterative mode.  k <= shortlist <= VSR_MAX_K; L2, inner product
 * and cosine; L1 is VSR_ERR_UNSUPPORTED.  Both stages run on the bit corpus context's stream with no host round trip; the
 * _device form does not synchronise, d_out_keys (may be NULL) receives the raw keys as vsr_search_quantized_device's does, and a
 * query whose LDS visited table overflowed (graphs beyond ~1M elements) has an empty shortlist there: count 0.  The host form
 * runs the call again with the global visited bitmap when that happens. */
int vsr_hnsw_search_quantized(vsr_corpus* source, vsr_hnsw* bit_index, const float* queries, int nq, int dim, int k, int shortlist,
                              int ef_search, int metric, const vsr_filter* const* filters,
                              int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist, int32_t* out_counts);
int vsr_hnsw_search_quantized_device(vsr_corpus* source, vsr_hnsw* bit_index, const float* d_queries, int nq, int dim, int k,
                                     int shortlist, int ef_search, int metric, const vsr_filter* const* filters,
                                     int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows, float* d_out_dist,
                                     int32_t* d_out_counts, uint64_t* d_out_keys);

/* The two-stage search through the IVFFlat index of the bits: CREATE INDEX ... USING ivfflat
 * ((binary_quantize(embedding)::bit(n)) bit_hamming_ops), ORDER BY ... <~> ... LIMIT shortlist under ivfflat.probes (and
 * ivfflat.iterative_scan / ivfflat.max_probes), then the re-rank on the original vectors.  bit_index is a vsr_ivf_load_bit index
 * over the corpus vsr_corpus_binary_quantize(source) made; source is fp32 or halfvec; the filters are filters of that bit corpus.
 * Per query q of `dim` floats:
 *   1. qb = binary_quantize(q), from the fp32 value as given: bit i is set where q[i] > 0 (NaN, 0 and -0.0 give 0);
 *   2. S = exactly the rows vsr_ivf_search_bit_iterative(bit_index, qb, k = shortlist, probes, VSR_METRIC_HAMMING, filters, mode,
 *      max_probes) returns: batches of `probes` lists in (Hamming count, list id) centre order, each batch contributing its
 *      (shortlist - have) smallest ((float) Hamming, document_id, block_id) keys, until `shortlist` rows are found or
 *      max(max_probes, probes) lists are scanned.  mode == VSR_IVF_ITERATIVE_OFF ignores max_probes and is vsr_ivf_search_bit's
 *      answer.  Stage 1 is one launch (K3q) that quantizes the queries itself and starts at the first list: no host planning;
 *   3. stage 2 is vsr_search_quantized's, unchanged: the exact operator distance on the source rows of S, the first
 *      min(k, |S|) returned, the same -1 / +Inf fill past out_counts[i].
 * out_probes (nq, may be NULL) receives the lists scanned, whole batches, as vsr_ivf_search_bit_iterative's.  out_rows and
 * out_doc_ids may be NULL.  k <= shortlist <= VSR_MAX_K; L2, inner product and cosine; L1 is VSR_ERR_UNSUPPORTED.
 * Consequences: with probes >= lists the call equals vsr_search_quantized(source, bits, ...); with a filter that admits at most
 * `shortlist` rows, VSR_IVF_ITERATIVE_RELAXED and max_probes >= lists it equals vsr_search(source) over those rows.
 * The _device form (queries nq x dim floats, row stride dim, 4-byte aligned, and all outputs in device memory) enqueues
 * everything on the bit corpus context's stream and does not synchronise; a filter's view-order bitmap is built, and waited
 * for, on its first use with this index only.  d_out_keys (nq*k, may be NULL) is as vsr_search_quantized_device's.  The host form
 * copies up, calls the device form's launches and copies down.
 * Errors.  bit_index not over a bit corpus: VSR_ERR_INVALID, "the index is not over a bit corpus (it is searched with
 * vsr_ivf_search*)".  Then vsr_search_quantized's checks against bit_index's corpus, in its words (bits not made from source,
 * shortlist < k, shortlist > VSR_MAX_K, L1, a filter of another corpus -- source's included --, VSR_ERR_DIM_MISMATCH).  probes,
 * mode and max_probes as vsr_ivf_search_iterative.  A shape whose LDS does not fit a compute unit: VSR_ERR_UNSUPPORTED. */
int vsr_ivf_search_quantized(vsr_corpus* source, vsr_ivf* bit_index, const float* queries, int nq, int dim, int k, int shortlist,
                             int probes, int metric, const vsr_filter* const* filters, int mode, int max_probes,
                             int64_t* out_block_ids, int32_t* out_doc_ids, int64_t* out_rows, float* out_dist,
                             int32_t* out_counts, int32_t* out_probes);
int vsr_ivf_search_quantized_device(vsr_corpus* source, vsr_ivf* bit_index, const float* d_queries, int nq, int dim, int k,
                                    int shortlist, int probes, int metric, const vsr_filter* const* filters, int mode,
                                    int max_probes, int64_t* d_out_block_ids, int32_t* d_out_doc_ids, int64_t* d_out_rows,
                                    float* d_out_dist, int32_t* d_out_counts, int32_t* d_out_probes, uint64_t* d_out_keys);

/* opclass support functions for n vectors at once (host pointers): vector_norm (vector.c:756-769), l2_normalize
 * (vector.c:774-808; fails with "value out of range: overflow" like float_overflow_error) and
 * vector_spherical_distance (vector.c:692-711; unit vectors assumed, as IVFFlat's spherical k-means uses it) */
int vsr_vector_norms(vsr_ctx* ctx, const float* a, int64_t n, int dim, double* out);
int vsr_l2_normalize(vsr_ctx* ctx, const float* a, int64_t n, int dim, float* out);
int vsr_spherical_distances(vsr_ctx* ctx, const float* a, const float* b, int64_t n, int dim_a, int dim_b, int b_broadcast,
                            double* out);

/* ---- measurement --------------------------------------------------------------------------------- */
typedef struct {
    /* K1 launches by kernel class: [0] = one query per pass, [1] = up to 4 queries sharing a pass */
    int64_t scan_launches[2];
    double  scan_ms[2];         /* sum of HIP-event durations of those launches          */
    int64_t scan_bytes[2];      /* algorithmic bytes: rows*dim*4 (halfvec corpus: *2; bit corpus: rows*((dim+7)/8); sparse corpus: 8 per stored entry) + bitmap bytes + k*12 */
    int64_t scan_rows[2];       /* rows scanned (per shared pass)                        */
    int64_t select_launches;    /* K5 */
    double  select_ms;
    int64_t queries;
    double  search_ms;          /* profiling level 1: device time of whole searches, staging kernel to last output kernel */
    /* ABI 2: what the launches HAD to do, whatever the pass structure (the honest roofline inputs) */
    int64_t scan_pairs[2];      /* (row, query) pairs = sum over passes of rows * queries: flops = 2 * dim * pairs       */
    int64_t unique_rows[2];     /* rows read at least once per launch, summed over launches: distinct filter parts'
                                   rows, capped at the corpus size (exact when the parts are disjoint, e.g. classes)  */
    /* host side of the search entry points (always on): time spent inside them, and the part of it spent WAITING for
       the previous batch's staging block (back-pressure from the GPU, not work) */
    double  host_ms;
    double  host_wait_ms;
} vsr_stats;

int vsr_profiling(vsr_ctx* ctx, int enable);      /* HIP events on the launch stream: 1 = around every launch class (scan, sample, K5), 2 = around the main scan launch only, 0 = off */
int vsr_stats_get(vsr_ctx* ctx, vsr_stats* out);  /* synchronises, accumulates pending events */
int vsr_stats_reset(vsr_ctx* ctx);
/* name of the kernel instantiation the main scan launch of the session's last search resolved to ("" before any); searches
   screened on the int8 planes append " + sample <kernel>", the instantiation of their sample launch */
int vsr_last_scan_kernel(vsr_ctx* ctx, char* name, int name_len);

/* launch-shape knobs (measurement only): blocks per launch budget, min rows per workgroup, queries per pass */
int vsr_tune(vsr_ctx* ctx, int block_budget, int min_rows_per_block, int max_queries_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* VSRBAC_H */
