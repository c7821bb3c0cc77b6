/* kmx.h — C-ABI of the MI355X-native k-mer exact-match batch search engine.
 *
 * This is the drop-in boundary underneath the reference's C++ template surface
 * (Clemapfel/kmer_index).  The reference has no FFI of its own; every entry point
 * below names the reference interface it stands in for (file:line relative to the
 * reference checkout).  The C++ host mirror in include/kmer_index_amd/ keeps the
 * reference's class and function names and calls only these functions.
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions cross the boundary: every call
 *     returns a kmx_status and kmx_last_error() gives a thread-local message;
 *   - letters are passed as alphabet RANKS, one byte per letter, exactly what
 *     seqan3::to_rank yields for the reference's alphabet_t (kmer_index.hpp:59,128);
 *   - positions are uint32_t text offsets (position_t = uint32_t, kmer_index.hpp:575);
 *   - input buffers are borrowed for the duration of the call; results are owned by
 *     the library until kmx_result_free;
 *   - one kmx_index may be searched from several host threads at once (the
 *     reference's search() is const, kmer_index.hpp:505) provided each call uses
 *     its own result handle (and, for the device-buffer form, its own stream): the
 *     host-buffer form runs on a stream owned by the result, so concurrent calls
 *     overlap on the GPU instead of queueing behind one another;
 *   - the engine needs the HIP runtime and a gfx950 device: there is no CPU path.
 */
#ifndef KMX_H
#define KMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMX_VERSION 5
#define KMX_MAX_KS 32               /* number of k values one index may hold                      */
#define KMX_MAX_DEVICES 16          /* replicas of one index (one per GPU of a node)              */
#define KMX_QUERY_SIZE_RANGE 10000  /* kmer_index::_query_size_range, kmer_index.hpp:401          */
#define KMX_SUBK_FANOUT_LIMIT 10000000ull /* sigma^(k-m) guard, kmer_index.hpp:119                */

typedef enum kmx_status {
    KMX_OK = 0,
    KMX_ERR_INVALID_ARGUMENT = 1,  /* bad pointer / size / k (static_assert kmer_index.hpp:42-43) */
    KMX_ERR_HIP = 2,               /* HIP runtime error (message has the HIP error string)       */
    KMX_ERR_OUT_OF_MEMORY = 3,
    KMX_ERR_NO_DEVICE = 4,         /* no gfx950 device visible: the engine never falls back       */
    KMX_ERR_TOO_LARGE = 5          /* text too long for 32-bit positions (kmer_index.hpp:169-170) */
} kmx_status;

/* Per-query status (array returned by kmx_result_status).  QUERY_TOO_LONG and
 * SUBK_FANOUT are the two places where the reference throws std::invalid_argument
 * (kmer_index.hpp:507-509 and :119-122); EMPTY_QUERY is its assert at :195. */
typedef enum kmx_query_status {
    KMX_Q_OK = 0,
    KMX_Q_TOO_LONG = 1,
    KMX_Q_SUBK_FANOUT = 2,
    KMX_Q_EMPTY_QUERY = 3,
    KMX_Q_BAD_RANK = 4,  /* a letter >= sigma: not representable in the reference's alphabet_t */
    KMX_Q_TOO_SHORT = 5  /* kmx_search_approx only: m <= max_subst letters, every window of the text would match */
} kmx_query_status;

/* How a query was served (array returned by kmx_result_kinds). */
typedef enum kmx_query_kind {
    KMX_KIND_NONE = 0,     /* error status or a part missed: empty result (kmer_index.hpp:204,224,524)  */
    KMX_KIND_EXACT = 1,    /* one bucket, bitmask bypassed (kmer_index.hpp:198-205, :529-530)           */
    KMX_KIND_STITCH = 2,   /* candidates = first part's bucket + validity mask (:207-339, :532-555)     */
    KMX_KIND_PREFIX = 3    /* m < k: every k-mer with this prefix + last-kmer fix-up (:115-148, :342-345) */
} kmx_query_kind;

typedef enum kmx_table_kind {
    KMX_TABLE_AUTO = 0,    /* dense when sigma^k <= 4 * (n-k+1), else open addressing                   */
    KMX_TABLE_OPEN = 1,    /* open-addressing {key, offset, count} slots, linear probing, load <= 0.5   */
    KMX_TABLE_DENSE = 2    /* direct addressing: offsets[sigma^k + 1]                                   */
} kmx_table_kind;

typedef struct kmx_options {
    uint32_t struct_size;  /* = sizeof(kmx_options)                                                     */
    int32_t device;        /* HIP device ordinal; -1 = current device                                   */
    uint32_t table_kind;   /* kmx_table_kind                                                            */
    uint32_t n_threads;    /* host threads for the per-k flatten (kmer_index ctor's n_threads, :481)    */
    uint32_t query_size_range; /* 0 = KMX_QUERY_SIZE_RANGE (extend_query_size_range, :498-502)          */
    uint32_t keep_host_arena;  /* keep a host copy of the position arena (kmx_index_arena_host)         */
    uint32_t host_flatten;     /* 1 = build every element on host threads; 0 = on the device when the
                                  key space allows (sigma^k <= 2^26), host otherwise                     */
    uint32_t no_aligned_copy;  /* 1 = keep neither of the derived bucket layouts: the second, 128-byte-line-aligned copy of
                                  long buckets (avg >= 32 positions; up to ~1.2x the position array, exact lookups read ~13 %
                                  less with it) and the fixed-size cells + one-byte count table of short buckets (avg <= 24;
                                  up to 8x the position array, +8...17 % queries/s on DNA5 k=10 / protein k=5).  Both are
                                  also left out on their own when their offsets would not fit 32 bits (texts near 2^32
                                  letters): kmx_index_info's device_bytes tells what an index really holds.          */
    /* ---- since KMX_VERSION 2 (a caller compiled against version 1 passes the shorter struct_size and gets one replica) ---- */
    uint32_t n_devices;        /* 0 / 1: one replica on `device`.  N > 1: the index is built once on devices[0] and its flat
                                  image replicated (device-to-device copies) into the HBM of devices[1..N-1]; a host-buffer
                                  batch search then shards the queries contiguously over the replicas — replica r gets queries
                                  [nq*r/N, nq*(r+1)/N) — and returns ONE result whose views concatenate the shards in replica
                                  order, byte for byte what one device returns (batches of fewer than 256 queries per
                                  replica go to the first replica whole).  0 also reads the environment
                                  variable KMX_DEVICES ("all" or a comma-separated list of ordinals), so that a caller of
                                  kmer::make_kmer_index uses every GPU of the node without a code change.  An ordinal may be
                                  listed more than once (replicas then share a device: only useful for testing).           */
    int32_t devices[KMX_MAX_DEVICES];
    /* ---- since KMX_VERSION 3 ---- */
    int32_t prefix_levels;     /* Sub-k queries (m < k, get_position_for_all_kmer_with_prefix kmer_index.hpp:115-148 + the std::sort
                                  of kmer_index_result.hpp:258): per dense element, up to this many PREFIX LEVELS are derived when
                                  the index is installed — level L holds, for every (k-L)-mer, the merged ascending list of all its
                                  occurrences, so a query of k-L letters copies one list instead of merging sigma^L buckets per
                                  query, and shorter ones merge sigma^L times fewer lists.  Results are identical; each level costs
                                  one more copy of the position array (4 bytes x text length) and is left out when it does not
                                  fit.  0 = default (KMX_PREFIX_LEVELS in the environment, else 2), -1 = none, N = at most N
                                  (<= 3).  Levels are derived data: not part of the on-disk image, rebuilt by kmx_index_load.
                                  A caller compiled against KMX_VERSION 1 or 2 (shorter struct_size: it cannot say what it
                                  wants) gets none.  kmx_index_levels reports what was built, kmx_index_memory what it costs. */
} kmx_options;

/* kmx_search_batch flags */
#define KMX_SEARCH_DEFAULT 0u
#define KMX_SEARCH_KEEP_MASKS 1u   /* keep candidate runs + compressed_bitset mask words for STITCH queries */
#define KMX_SEARCH_COUNT_ONLY 2u   /* stop after hit_off (no position lists are materialised)              */
#define KMX_SEARCH_ASYNC 4u        /* device form only: return once the first half of the search is enqueued (lookup,
                                      scan, the steady-state fill) without waiting for the counters; the search is
                                      completed by whatever touches the result next (counts / view / masks / free / a
                                      new search into it, or kmx_index_free of its index, which completes every search
                                      still pending on the index before it releases anything).  d_qranks and d_qoff must
                                      stay alive until then.  Two results used in turn keep the GPU busy across batches. */
#define KMX_SEARCH_REFERENCE_PLAN 8u /* answer every query from the element the REFERENCE's planner names (choose_search_scheme,
                                      kmer_index.hpp:407-476).  By default a single-k query longer than its k is answered from
                                      the largest k of the index that fits it instead of the k that wastes the fewest letters
                                      (kmer_index.hpp:465-473): the buckets to intersect are shorter by sigma^(difference) and
                                      the position lists are the same — but which of KMX_KIND_NONE / KMX_KIND_STITCH a query
                                      WITHOUT hits reports may differ (an absent part of the larger k ends the lookup early).
                                      KMX_SEARCH_KEEP_MASKS implies this flag: candidate runs and mask words are the
                                      reference's result object.  kmx_plan always reports the reference's tables.           */

typedef struct kmx_index kmx_index;
typedef struct kmx_result kmx_result;

/* Per-kernel timing collected with HIP events on the caller's stream. */
#define KMX_N_KERNELS 16
typedef struct kmx_kernel_stat {
    const char* name;
    uint64_t launches;
    double total_ms;
} kmx_kernel_stat;

/* ---- construction: stands in for kmer::make_kmer_index<ks...>(text, n_threads)
 *      (kmer_index.hpp:569-579) and the kmer_index constructor (:480-496), i.e. one
 *      kmer_index_element::create per k (:154-179) plus choose_search_scheme (:407-476).
 *      `ranks` holds n letters as ranks < sigma.  Requires 0 < k < 64/log2(sigma) for
 *      every k (:42-43), n >= max k and n + max k - 1 < 2^32 (:169-170). */
kmx_status kmx_index_build(const uint8_t* ranks, uint64_t n, uint32_t sigma, const uint32_t* ks,
                           uint32_t n_ks, const kmx_options* opts, kmx_index** out);
void kmx_index_free(kmx_index* index);

/* On-disk image of the flattened index: build once, load many (the intent stated in the thesis,
 * thesis/content/02_implementation.tex:44-46; not implemented by the reference).  kmx_index_load validates
 * magic, version, every size field (the file must be exactly as long as its element table says — nothing is
 * allocated on the word of a header the file cannot back) and a checksum, and then the CONTENTS the kernels index
 * with — group boundaries monotone and ending at npos, the positions of every group strictly ascending and inside
 * the text, distinct keys strictly ascending and inside the key space, at most half of the open-addressing slots
 * occupied (a full table would make the probe loop spin), every slot naming exactly the group of its key, the
 * aligned copy restating the groups, the text tail inside the alphabet — before touching the device.  An image
 * that loads can be searched without harm whatever else it holds (tests/test_image_cpu.py, test_image_gpu.py:
 * mutation fuzz). */
kmx_status kmx_index_save(const kmx_index* index, const char* path);
kmx_status kmx_index_load(const char* path, const kmx_options* opts, kmx_index** out);

/* Introspection of the flattened index (sizes in bytes are device-resident bytes). */
kmx_status kmx_index_info(const kmx_index* index, uint64_t* n, uint32_t* sigma, uint32_t* n_ks,
                          uint32_t* ks /* KMX_MAX_KS */, uint32_t* table_kinds /* KMX_MAX_KS */,
                          uint64_t* device_bytes);

/* What the device memory of one replica (kmx_index_info's device_bytes) is made of, in bytes: the position arrays proper
 * (4 bytes per k-mer start and element — the reference's buckets), and the layouts DERIVED from them that an options field or
 * an environment variable turns off: the 128-byte-line-aligned copy of long buckets and the cells of short ones
 * (no_aligned_copy), the prefix levels (prefix_levels); `tables` is the rest (offset / slot / key tables, directories, padding,
 * planner tables, tail).  Any pointer may be NULL. */
kmx_status kmx_index_memory(const kmx_index* index, uint64_t* positions, uint64_t* aligned_copy, uint64_t* cells,
                            uint64_t* prefix_levels, uint64_t* tables);

/* kmer_index::extend_query_size_range(new_maximum) (kmer_index.hpp:498-502): rebuilds the planner
 * table for query lengths < new_maximum and installs it.  Must not run concurrently with a search
 * on the same index. */
kmx_status kmx_index_extend_query_size_range(kmx_index* index, uint32_t new_maximum);

/* Planner tables — kmer_index::_optimal_nk_sum / _use_multi_search_scheme
 * (kmer_index.hpp:404-405) as built by choose_search_scheme (:407-476).  Pure host
 * code; usable without a device.  nk_off has range+1 entries into nk_flat; returns
 * the number of flat entries through *n_flat (call with nk_flat = NULL to size). */
kmx_status kmx_plan(const uint32_t* ks, uint32_t n_ks, uint32_t range, uint8_t* use_multi,
                    uint32_t* nk_off, uint32_t* nk_flat, uint64_t cap, uint64_t* n_flat);

/* The ENGINE's choice of element per query length (see KMX_SEARCH_REFERENCE_PLAN): k_used[q], q < range, is the k whose
 * element answers a query of q letters that the reference plans on ONE k — the reference's k for q <= k, exact multiples that
 * have no larger k to go to, and lengths whose rest could reach the sub-k fan-out guard on either choice; otherwise the largest
 * k of the index that fits q.  0 for lengths the reference answers with its multi-k scheme (their summands are kmx_plan's) and
 * for q == 0.  Pure host code; what a search without KMX_SEARCH_KEEP_MASKS / KMX_SEARCH_REFERENCE_PLAN runs on. */
kmx_status kmx_plan_engine(const uint32_t* ks, uint32_t n_ks, uint32_t range, uint32_t sigma, uint32_t* k_used);

/* choose_best_k (choose_best_k.hpp:12-60): the n_k (<= 10) values of k the reference's heuristic recommends for a
 * set of query lengths — candidates {29,27,25,23,21,19,17,13,11,10}, 3 points for a length the candidate divides,
 * 4 - miss points for a miss of at most 3, best scores first.  Pure host code. */
kmx_status kmx_choose_best_k(const uint64_t* query_lengths, uint64_t n_lengths, uint32_t n_k, uint32_t* ks_out);

/* kmer::detail::fast_pow (fast_pow.hpp:46-93), including its "0 on exp >= 63" rule. */
uint64_t kmx_fast_pow(uint64_t base, uint8_t exp);

/* ---- search: stands in for kmer_index::search(std::vector<alphabet_t>&) const
 *      (kmer_index.hpp:505-558) applied to a BATCH of queries, followed by
 *      kmer_index_result::to_vector() (kmer_index_result.hpp:244-260) per query.
 *      qranks: the queries' letters as ranks, concatenated; qoff[nq+1]: start of each
 *      query in qranks (qoff[0] = 0; qranks may be NULL when no query has a letter).  Host-buffer form:
 *      copies the inputs to the device, runs the device form on a stream owned by the result, and
 *      leaves the result ready for kmx_result_view.  Small batches (up to 8192 queries that are mostly
 *      plain lookups; kmer_index::search(query) is a batch of one) take a latency path instead: ONE launch
 *      that reads the queries from and writes the complete result to page-locked host memory — no copies,
 *      one wait (about 17-30 us for one query).  Such a result lives in host memory; kmx_result_view_device
 *      on it runs the device form then (the index must still exist). */
kmx_status kmx_search_batch(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff,
                            uint64_t nq, uint32_t flags, kmx_result** out);
/*      A batch whose descriptors or hit lists do not fit the device in one pass (more than 2^25 queries, or an out-of-memory
 *      on the first attempt) is streamed through the device in chunks: every chunk's result is moved to host memory and the
 *      device buffers serve the next chunk, a chunk that still does not fit is halved.  The result then has one part per
 *      chunk (kmx_result_parts), its host views and counts are those of the whole batch, device views do not exist for it. */

/* Device-buffer form: d_qranks / d_qoff are device pointers already resident in HBM (on an index with several replicas: in
 * the HBM of any of its devices — the replica on the device that owns d_qranks serves the call),
 * `stream` is a hipStream_t (NULL = the default stream).  All kernels are enqueued on
 * `stream`; the call returns after the one host read-back it needs (per-kind counts
 * and the hit total, 64 bytes) and with the fill kernels enqueued.  Passing a result
 * from a previous call in *inout reuses its device buffers (no allocation in the
 * steady state). */
kmx_status kmx_search_batch_device(const kmx_index* index, const void* d_qranks, const void* d_qoff,
                                   uint64_t nq, uint32_t flags, void* stream, kmx_result** inout);

/* Result access.  Device views are valid after the call returns (in stream order);
 * host views copy to pinned host memory on first use and synchronise the stream.
 *   hit_off[nq+1]  : start of query q's hits in `positions` (uint64)
 *   positions[...] : per query the ascending list of text offsets where it occurs —
 *                    kmer_index_result::to_vector() (kmer_index_result.hpp:244-260)
 *   status[nq]     : kmx_query_status (uint8)
 *   kinds[nq]      : kmx_query_kind   (uint8) */
kmx_status kmx_result_counts(const kmx_result* r, uint64_t* nq, uint64_t* n_hits, uint64_t* n_exact,
                             uint64_t* n_stitch, uint64_t* n_prefix, uint64_t* n_error);
kmx_status kmx_result_view_device(const kmx_result* r, const uint64_t** d_hit_off,
                                  const uint32_t** d_positions, const uint8_t** d_status);
kmx_status kmx_result_view(kmx_result* r, const uint64_t** hit_off, const uint32_t** positions,
                           const uint8_t** status, const uint8_t** kinds);

/* Multi-device results.  A result of a host-buffer search on an index with N replicas has N parts, part p holding
 * the queries [q_begin, q_end) on `device`; kmx_result_view / kmx_result_masks / kmx_result_counts present the parts as one
 * result, kmx_result_view_device is refused for N > 1 (there is no single device to point into) — use the per-part device
 * views, whose hit_off is local to the part (hit_off[0] == 0).  Every other result has exactly one part. */
kmx_status kmx_result_parts(const kmx_result* r, uint32_t* n_parts);
kmx_status kmx_result_part_view_device(const kmx_result* r, uint32_t part, int32_t* device, uint64_t* q_begin, uint64_t* q_end,
                                       const uint64_t** d_hit_off, const uint32_t** d_positions, const uint8_t** d_status);
/* The devices an index is replicated on (devices[] holds KMX_MAX_DEVICES entries). */
kmx_status kmx_index_devices(const kmx_index* index, uint32_t* n_devices, int32_t* devices);

/* The exchange step of SURVEY 8e behind the C-ABI ("hit lists gathered ... over xGMI"): the parts of a multi-device result
 * gathered into ONE set of device arrays in the HBM of `dst_device` (any device of the node; normally the first replica's):
 * every part's hit lists go device to device (hipMemcpyPeerAsync on the part's own stream — all links at once, each behind
 * its part's last kernel) to the displacement the parts in front of it leave, its hit_off entries are rebased by that
 * displacement on the destination, its statuses follow.  What arrives is byte for byte what one device returns for the whole
 * batch: d_hit_off[nq + 1] (global), d_positions[n_hits], d_status[nq].  The arrays belong to the result (freed with it,
 * reused by the next gather into it) and are complete when the call returns.  A single-part result on dst_device is
 * returned where it lies (no copy).  Refused for chunk-streamed results (they live in host memory) and COUNT_ONLY
 * searches have no positions (d_positions = NULL). */
kmx_status kmx_result_gather_device(kmx_result* r, int32_t dst_device, const uint64_t** d_hit_off, const uint32_t** d_positions,
                                    const uint8_t** d_status);

/* KMX_SEARCH_KEEP_MASKS only — the reference's zero-copy result view
 * (kmer_index_result.hpp:15-24: pointers to bucket vectors + a compressed_bitset).
 * For a STITCH query q (kinds[q] == KMX_KIND_STITCH):
 *   cand_src[q]   : arena index of its candidate run = the first part's bucket
 *                   (kmer_index.hpp:272, :532), cand_count[q] ascending positions;
 *   mask_base[q]  : index of its first word in mask_words; it owns
 *                   cand_count[q]/64 + 1 words in compressed_bitset layout
 *                   (compressed_bitset.hpp:9-105: bit i = word i>>6, bit i&63);
 *                   bit i set <=> candidate i is a hit; padding bits are 0.
 * Entries of other queries are undefined.  The arena itself is reachable on the
 * host through kmx_index_arena_host when the index was built with keep_host_arena. */
kmx_status kmx_result_masks(kmx_result* r, const uint64_t** mask_base, const uint64_t** mask_words,
                            const uint32_t** cand_count, const uint64_t** cand_src);
kmx_status kmx_index_arena_host(const kmx_index* index, const uint32_t** arena, uint64_t* n_elems);

/* kmer_index_element<alphabet_t, position_t, k>::search_k(iterator) (kmer_index.hpp:183-190) = at(hash(it)) (:56-84): the
 * bucket of ONE k-mer, as a borrowed window into the index's host arena — no device round trip, nothing to free; valid as
 * long as the index.  `ranks` holds the k letters; *positions / *count receive the ascending text offsets of that k-mer,
 * NULL / 0 when the text does not hold it (the reference's nullptr).  Needs keep_host_arena; the element's offset table
 * (dense: 4 bytes per key; open addressing: 12 bytes per distinct key) is mirrored to host memory by the first call that
 * asks for that k.  Callable from several threads at once.  KMX_ERR_INVALID_ARGUMENT: no element for this k, a letter
 * outside the alphabet, an index without host arena. */
kmx_status kmx_index_bucket_host(const kmx_index* index, uint32_t k, const uint8_t* ranks, const uint32_t** positions,
                                 uint32_t* count);

/* Prefix levels actually built (kmx_options::prefix_levels asks, memory and the planner decide): levels[i] = number of levels
 * of the element of ks[i] (kmx_index_info's order), 0 for elements without.  levels holds KMX_MAX_KS entries. */
kmx_status kmx_index_levels(const kmx_index* index, uint32_t* levels);

/* Which code path ran (an extension, read-only; a caller detects the capability by the macro KMX_PATH_INFO, KMX_VERSION is
 * unchanged).  Several kernels of the exact search exist in variants chosen from the index (arena size, bucket density), from
 * what the previous batch on the result handle held, or from tuning variables in the environment (KMX_FILL_VARIANT,
 * KMX_FORCE_REC64, KMX_CELLS, KMX_CELL_SHIFT read when an index is installed; KMX_LOOKUP_ITEMS, KMX_NO_SMALL read once per
 * process); a value those variables do not recognise leaves the default in place.  Results never depend on the choice; these
 * two calls report it, so that a test or a tuning run knows what it measured.  The caller sets struct_size = sizeof(the
 * struct); the library fills the fields that size covers. */
#define KMX_PATH_INFO 1
typedef struct kmx_index_path_info {
    uint32_t struct_size;
    uint32_t fill_slots;        /* output slots per thread of k_fill as launched: 4, 8, 12 or 16 (tile = 256 x this)          */
    uint32_t fill_nontemporal;  /* k_fill writes the hit lists with non-temporal stores                                      */
    uint32_t rec64;             /* k_fill keeps 64-bit records (arenas of 4 GiB or more; always 8 slots per thread)          */
    uint32_t tiny_cells;        /* some element has cells and at most four positions per key: k_lookup takes 8 queries per
                                   thread on batches without cross-referenced queries                                       */
    uint32_t scan_tile;         /* queries per block of the scan over the hit counts (a multiple of every lookup block)      */
    uint32_t n_ks;
    uint32_t cell_shift[KMX_MAX_KS]; /* per element (kmx_index_info's order): log2 of its cell size in positions, 0 = no cells */
    uint32_t windows_tile;      /* windows per block of k_lookup_windows (kmx_search_windows): a divisor of scan_tile         */
} kmx_index_path_info;
kmx_status kmx_index_paths(const kmx_index* index, kmx_index_path_info* out);

/* The last finished search into `r` (a pending KMX_SEARCH_ASYNC search is completed first).  Refused for results of several
 * parts (multi-device, chunk-streamed): every part ran a search of its own. */
typedef struct kmx_result_path_info {
    uint32_t struct_size;
    uint32_t small;             /* the latency path answered (k_small): every field below is 0                               */
    uint32_t lookup_items;      /* queries per thread of k_lookup: 4 or 8                                                    */
    uint32_t lookup_pairs;      /* k_lookup ran the variant that interleaves cross-referenced (two-part) queries             */
    uint32_t deferred_long;     /* queries of very many parts were listed by k_lookup and served by k_lookup_long            */
    uint32_t tile_q_source;     /* who wrote the first query of every output tile for the k_fill whose output was kept:
                                   KMX_TILE_Q_NONE (no fill: no hits, KMX_SEARCH_COUNT_ONLY), _PARTITION (k_partition: first
                                   batch of a handle, or its tile table had to grow) or _SCAN (the scan's downsweep)          */
    uint32_t spec_fill;         /* k_fill was launched behind the scan, before the host knew the hit total                   */
    uint32_t spec_ok;           /* ... and its output was kept (no second k_fill; also when the batch has no hits at all)    */
    uint32_t fill_blocks;       /* grid of the k_fill whose output was kept (blocks beyond the hit total leave at once)      */
    uint32_t fill_tiles;        /* tiles that hold hits: ceil(n_hits / (256 x fill_slots))                                   */
    /* The batch's sub-k (KMX_KIND_PREFIX) queries by the merger their slice went to (len = positions of the slice without the
     * last-kmer positions, R = its runs), from the counters the search reads back anyway:                                    */
    uint32_t prefix_plain;       /* R < 2 or len < 2: one list (a prefix level's, or the only key), copied as it lies        */
    uint32_t prefix_small;       /* len <= 2048, not of the next class: k_prefix_sort_small (one wave)                        */
    uint32_t prefix_merge_small; /* len <= 2048, 2 .. 32 runs of 8 positions or more on average, beyond 4 runs / 512
                                    positions: k_prefix_merge_small                                                          */
    uint32_t prefix_mid;         /* 2048 < len <= 8192: k_prefix_sort_block, a block per slice                                */
    uint32_t prefix_long;        /* len > 8192: one chunk (len <= 32768) or, beyond, value bands, a spread by value or chunks
                                    + merge passes — which of the three is decided on the device and not read back           */
    uint32_t prefix_large_chunks;/* the most chunks of 32768 positions any slice of the batch has (0: no slice beyond one)    */
    uint64_t prefix_large_elems; /* positions of the slices beyond one chunk (len > 32768), summed                            */
} kmx_result_path_info;
#define KMX_TILE_Q_NONE 0u
#define KMX_TILE_Q_PARTITION 1u
#define KMX_TILE_Q_SCAN 2u
kmx_status kmx_result_paths(const kmx_result* r, kmx_result_path_info* out);

void kmx_result_free(kmx_result* r);

/* ---- approximate search: an extension, no reference interface.  Every window of the text within Hamming distance
 *      max_subst (substitutions only, no insertions or deletions) of each query of a batch.
 *
 * For a query q of m letters and e = max_subst (0 <= e <= KMX_APPROX_MAX_SUBST) the result holds the strictly ascending list
 * of every text offset p with p + m <= n and Hamming(text[p, p + m), q) <= e, and for each such offset its number of
 * mismatches.  The query is cut into e + 1 pieces (the first m mod (e + 1) one letter longer than the others); by the
 * pigeonhole principle one piece of every such window matches exactly, so the pieces go through the exact batch search
 * (kmx_search_batch_device, any piece length: exact, stitched, sub-k, multi-k) and each piece hit is verified against a
 * packed copy of the text on the device.  Per-query status (kmx_query_status, uint8), in this order of precedence:
 * KMX_Q_EMPTY_QUERY for m = 0; KMX_Q_TOO_SHORT for m <= e; KMX_Q_TOO_LONG when the longest piece, ceil(m / (e + 1))
 * letters, reaches the index's query size range; KMX_Q_BAD_RANK for a letter >= sigma; KMX_Q_SUBK_FANOUT when the exact
 * search of a piece reports it.  Every status but KMX_Q_OK comes without hits; m > n is KMX_Q_OK without hits.
 * With e = 0 the positions are those of kmx_search_batch for every query it answers with KMX_Q_OK.
 *
 * Host buffers in (qranks / qoff as for kmx_search_batch), a host-resident result out.  The batch is streamed through
 * the device in chunks of queries whose piece hits fit a candidate budget and whose pieces number at most 2^25 (the
 * environment variables KMX_APPROX_CHUNK_CANDIDATES and KMX_APPROX_CHUNK_PIECES, read at every call, lower the two
 * bounds); the views always cover the whole batch.  Each call
 * runs on a stream and device buffers of its own: concurrent calls on one index are safe.  On an index with several
 * replicas the call runs on the first replica (batches are not sharded over replicas).  flags: 0 or KMX_APPROX_EDIT; any
 * other bit is refused.  The call searches the strand the index was built from; kmx_search_approx_strands (below)
 * searches the reverse complement of every query as well.
 *
 * KMX_APPROX_EDIT (a caller detects the capability by the macro; KMX_VERSION is unchanged): edit distance with unit costs
 * (substitution, insertion, deletion) in place of Hamming distance, max_subst read as the bound e on edits.  A start offset
 * p (0 <= p < n) is a hit when some window text[p, p + L) with L >= 1 and p + L <= n has Levenshtein distance <= e to q
 * (only L in [m - e, m + e] can qualify).  Per hit, mismatches[] of kmx_approx_view holds d(p), the least such distance, and
 * kmx_approx_lengths gives L(p): among the L that reach d(p) the one nearest to m, the shorter of two equally near.  Per
 * query the hits are strictly ascending in p, each once; every start is reported, the neighbours of a good alignment
 * included (p +- 1 at distance d + 1, and so on).  Statuses and their precedence are those above; m > n is served and has
 * hits when some window of at least m - e letters qualifies.  With e = 0 the positions are those of the call without the
 * flag, distances 0 and lengths m; for every e the hits without the flag are a subset, none with a smaller mismatch
 * count than its d(p).  The pieces and their exact search are the same: a window within e edits holds one piece exactly, at
 * most e letters off its nominal offset, so every piece hit names 2e + 1 candidate starts, verified by a banded dynamic
 * programme on the device, deduplicated and ordered there.  n_candidates still counts piece hits; each of them counts
 * 2e + 1 times against the candidate budget of a chunk. */
#define KMX_APPROX_MAX_SUBST 3
#define KMX_APPROX_EDIT 1u
typedef struct kmx_approx_result kmx_approx_result;
kmx_status kmx_search_approx(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq,
                             uint32_t max_subst, uint32_t flags, kmx_approx_result** out);
/* n_chunks: how many chunks the batch was streamed in (1 when it fit).  Any pointer may be NULL. */
kmx_status kmx_approx_counts(const kmx_approx_result* r, uint64_t* nq, uint64_t* n_hits, uint64_t* n_candidates,
                             uint32_t* n_chunks);
/*   hit_off[nq+1] : start of query q's hits (uint64); positions[n_hits] (uint32), mismatches[n_hits] (uint8) and
 *   status[nq] (uint8).  Valid until kmx_approx_free. */
kmx_status kmx_approx_view(kmx_approx_result* r, const uint64_t** hit_off, const uint32_t** positions,
                           const uint8_t** mismatches, const uint8_t** status);
/*   lengths[n_hits] (uint32), parallel to positions: the window length L(p) of every hit of a KMX_APPROX_EDIT call;
 *   KMX_ERR_INVALID_ARGUMENT on the result of a call without the flag.  Valid until kmx_approx_free. */
kmx_status kmx_approx_lengths(kmx_approx_result* r, const uint32_t** lengths);
void kmx_approx_free(kmx_approx_result* r);

/* ---- both strands: kmx_search_approx on every query AND on its reverse complement, in one call (an extension; a caller
 *      detects the capability by the macro KMX_APPROX_BOTH_STRANDS, KMX_VERSION is unchanged).
 *
 * Complement table.  The engine knows ranks, not letters, so the caller supplies `complement`: sigma entries that map rank
 * to rank.  It must be an involution on [0, sigma): complement[r] < sigma and complement[complement[r]] == r.  A NULL table,
 * one that is not an involution, or an entry >= sigma returns KMX_ERR_INVALID_ARGUMENT.  The identity is allowed: it
 * searches the plain reversal.
 * Reverse complement.  For a query q of m letters, rc(q)[i] = complement[q[m - 1 - i]].
 * What is reported.  Everything kmx_search_approx with the same max_subst and flags (0 or KMX_APPROX_EDIT; any other bit is
 * refused) reports for q, tagged strand 0, and everything that call reports for rc(q), tagged strand 1.  Offsets are always
 * offsets into the indexed (forward) text: for a reverse hit, the start of the window that rc(q) matches; its mismatch count
 * or distance, and with KMX_APPROX_EDIT its length L(p), are those of rc(q) at that start.
 * Order.  Per query the hits are strictly ascending in (position, strand): an offset may appear twice, forward first.
 * Nothing is deduplicated across strands: a query equal to its own reverse complement reports every hit on both.
 * Statuses and their precedence are those of kmx_search_approx.  A query is served only if both strands are: it takes the
 * forward strand's status unless that is KMX_Q_OK, otherwise the reverse strand's (only KMX_Q_SUBK_FANOUT can differ between
 * the two).  Every status but KMX_Q_OK comes without hits on either strand.
 * Accessors.  kmx_approx_counts (n_hits and n_candidates cover both strands), kmx_approx_view and, for a KMX_APPROX_EDIT
 * call, kmx_approx_lengths work on the result as on one of kmx_search_approx; kmx_approx_strands gives strands[n_hits]
 * (uint8, parallel to positions: 0 = forward, 1 = reverse; valid until kmx_approx_free) and returns
 * KMX_ERR_INVALID_ARGUMENT on a result of plain kmx_search_approx.
 * Chunking.  The budgets and the two environment variables work as for kmx_search_approx; a query and its reverse complement
 * are never split across chunks, KMX_APPROX_CHUNK_PIECES bounds the pieces of both strands together (2 (e + 1) per query),
 * and a query counts the piece hits of both strands against the candidate budget.
 * The reads cross to the device once; the reverse complements are made there, both strands go through the pipeline of
 * kmx_search_approx as one batch of 2 nq queries and the two hit lists of a query are merged on the device.  Concurrent calls
 * on one index are safe; the call runs on the first replica.  With e = 0 the strand-0 positions of a query are those
 * kmx_search_batch gives for q and the strand-1 positions those it gives for rc(q), for every query that call answers with
 * KMX_Q_OK. */
#define KMX_APPROX_BOTH_STRANDS 1
kmx_status kmx_search_approx_strands(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq,
                                     uint32_t max_subst, uint32_t flags, const uint8_t* complement,
                                     kmx_approx_result** out);
kmx_status kmx_approx_strands(kmx_approx_result* r, const uint8_t** strands);

/* ---- reporting: one hit per alignment locus, the best stratum only, at most N hits per query (an extension; a caller
 *      detects the capability by the macro KMX_APPROX_REPORT, KMX_VERSION is unchanged).  The familiar form is
 *      `-k N --best --strata` of a read mapper.  The filtering runs on the device, in front of the copy to the host.
 *
 * kmx_search_approx_opts takes its arguments in a struct: max_subst as kmx_search_approx; flags, any of KMX_APPROX_EDIT,
 * KMX_APPROX_LOCI and KMX_APPROX_BEST; max_hits, the cap (0 = none); complement, NULL for the strand the index was built
 * from (kmx_search_approx), otherwise the table of kmx_search_approx_strands, and both strands are searched.  struct_size must
 * be at least sizeof(kmx_approx_options).  Refused with KMX_ERR_INVALID_ARGUMENT before any device is touched: NULL
 * options, a smaller struct_size, any other flag bit, KMX_APPROX_LOCI without KMX_APPROX_EDIT (Hamming hits cast no
 * shadows), max_subst > KMX_APPROX_MAX_SUBST, and a bad complement table as kmx_search_approx_strands refuses it.
 * kmx_search_approx and kmx_search_approx_strands keep refusing every flag bit but KMX_APPROX_EDIT.
 *
 * What is reported.  Let H(q) be the hit list of query q that the call reports with KMX_APPROX_LOCI and KMX_APPROX_BEST
 * cleared and max_hits = 0: exactly the list of kmx_search_approx (complement == NULL) or kmx_search_approx_strands with the
 * same max_subst and KMX_APPROX_EDIT bit; with no option set the call returns that result array for array and does no further
 * work on the device.  A hit is (p, strand, d, L): offset, strand (0 throughout for one strand), mismatches or distance,
 * window length (edit only).  e = max_subst.  Three steps, in this order:
 *   1. KMX_APPROX_LOCI.  A hit (p, s, d) survives unless H(q) holds a hit (p', s, d') on the same strand with p' != p,
 *      |p' - p| <= e and (d', p') < (d, p) lexicographically.  The rule looks at H(q), not at the survivors: a hit removed by
 *      a better neighbour still removes its own worse neighbours.  A start at distance d casts its shadows (p +- i at distance
 *      d + i) no farther than e - d away, so the radius e removes all of them; of equal distances within the radius the
 *      leftmost stays.  Hits on different strands never suppress each other.  With e = 0 nothing is removed.
 *   2. KMX_APPROX_BEST.  Of the survivors, those whose d equals the least d among the query's survivors; with both strands
 *      the least d over both strands together.
 *      Steps 1 and 2 commute: the least d of H(q) is always the d of a survivor of step 1 (on each strand the least (d, p)
 *      has nothing below it), and a hit of that stratum can only be removed by a hit of that stratum, so step 1 applied to
 *      the best stratum of H(q) leaves the same hits.
 *   3. The cap.  found[q] (kmx_approx_found) is the number of hits left after steps 1 and 2.  With max_hits != 0 and
 *      found[q] > max_hits, the max_hits hits that come first in (d, p, strand) order are kept.
 * The hits kept are reported in the usual order, strictly ascending in (position, strand), each with the d, L and strand it
 * has in H(q).  A caller sees truncation as found[q] > hit_off[q + 1] - hit_off[q].
 * Unchanged: the statuses and their precedence, n_candidates, the chunk budgets and the two environment variables, and the
 * rule that a query (both strands of it) is never split across chunks, so every step sees the whole of H(q).
 * kmx_approx_counts gives in n_hits the hits returned (the length of positions[]); kmx_approx_view, kmx_approx_lengths and
 * kmx_approx_strands work as on the results of the older entry points, the latter two refused without KMX_APPROX_EDIT /
 * without a complement table.
 * kmx_approx_found: found[nq] (uint64), valid until kmx_approx_free, on every result of kmx_search_approx_opts (without a
 * cap it equals the list lengths); KMX_ERR_INVALID_ARGUMENT on a result of kmx_search_approx or kmx_search_approx_strands.
 * Accessors of one result are not to be called concurrently. */
#define KMX_APPROX_REPORT 1
#define KMX_APPROX_LOCI 2u /* needs KMX_APPROX_EDIT */
#define KMX_APPROX_BEST 4u
typedef struct kmx_approx_options {
    uint32_t struct_size;      /* = sizeof(kmx_approx_options) */
    uint32_t max_subst;        /* as kmx_search_approx */
    uint32_t flags;            /* KMX_APPROX_EDIT | KMX_APPROX_LOCI | KMX_APPROX_BEST */
    uint32_t max_hits;         /* 0 = no cap; else at most this many hits per query */
    const uint8_t* complement; /* NULL = one strand; else both, as kmx_search_approx_strands */
} kmx_approx_options;
kmx_status kmx_search_approx_opts(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq,
                                  const kmx_approx_options* options, kmx_approx_result** out);
kmx_status kmx_approx_found(kmx_approx_result* r, const uint64_t** found /* [nq] */);

/* ---- every k-mer window of a batch of reads in one call: an extension, no reference interface (a caller detects the
 *      capability by the macro KMX_SEARCH_WINDOWS, KMX_VERSION is unchanged).  What seeding a read mapper, k-mer containment and
 *      read classification ask of the index is "where does this k-mer occur" for EVERY k-mer of every read; written out as
 *      separate queries for kmx_search_batch that is len - k + 1 queries per read, each letter k times and 8 bytes of offset per
 *      window.  These calls take the reads as they are.
 *
 *      ranks / roff[nr+1] are shaped like qranks / qoff: roff[0] = 0, ranks may be NULL when no read has a letter.  Read r has
 *      len_r = roff[r+1] - roff[r] letters and contributes c_r = 0 windows if len_r < w, otherwise (len_r - w) / stride + 1;
 *      window j of read r is ranks[roff[r] + j*stride, +w).  win_off[nr+1] is the exclusive prefix sum of c_r: window j of read
 *      r is query win_off[r] + j of the result, and nq = win_off[nr].  The result is an ordinary kmx_result: kmx_result_counts,
 *      kmx_result_view and kmx_result_view_device give hit_off[nq+1], positions, status[nq] and kinds[nq] array for array what
 *      kmx_search_batch returns for the batch of those nq windows written out as separate queries, with the same flags.
 *      Statuses are therefore KMX_Q_OK or KMX_Q_BAD_RANK (a window with a letter >= sigma), kinds KMX_KIND_EXACT or
 *      KMX_KIND_NONE.  kmx_result_paths on such a result reports 0 in the k_lookup and prefix fields, the fill fields as usual.
 *
 *      Refused with KMX_ERR_INVALID_ARGUMENT before any device is touched: a NULL index, options or result pointer, a
 *      struct_size that is too small, stride == 0, any flag bit other than KMX_SEARCH_COUNT_ONLY (KEEP_MASKS, ASYNC and
 *      REFERENCE_PLAN have nothing to act on), a w that is not the k of an element of the index.  Refused after counting:
 *      nq >= 2^32 - 1, and a single read with 2^32 or more windows.
 *
 *      Host form: uploads the reads and roff once — no copy with the windows written out is made on either side —, computes nq
 *      on the host and runs the device form on a stream owned by the result.  It does not take the small-batch latency path and
 *      does not stream in chunks: when the descriptors or hit lists do not fit the device it returns KMX_ERR_OUT_OF_MEMORY and
 *      the caller splits the reads.  On an index with several replicas it runs on the first one.  *out as for kmx_search_batch
 *      (NULL, or a handle to reuse).
 *
 *      Device form: d_ranks / d_roff are device pointers, all kernels go on `stream`, the replica is the one on the device
 *      that owns d_ranks (as kmx_search_batch_device).  *inout reuses a handle's buffers; it is the handle type of
 *      kmx_search_batch_device, and searches of both kinds may alternate on one handle.  The call costs one 8-byte read-back
 *      (the window total) more than kmx_search_batch_device.
 *
 *      kmx_result_window_offsets: win_off on the host (copied on first use, valid until the handle is searched into again or
 *      freed) and / or on the device, and nr; any pointer may be NULL.  KMX_ERR_INVALID_ARGUMENT on a result that is not from a
 *      windows call. */
#define KMX_SEARCH_WINDOWS 1
typedef struct kmx_window_options {
    uint32_t struct_size;   /* = sizeof(kmx_window_options) */
    uint32_t w;             /* window length: must equal the k of one element of the index */
    uint32_t stride;        /* >= 1: windows start at offsets 0, stride, 2*stride, ... of each read */
    uint32_t flags;         /* KMX_SEARCH_DEFAULT or KMX_SEARCH_COUNT_ONLY */
} kmx_window_options;
kmx_status kmx_search_windows(const kmx_index* index, const uint8_t* ranks, const uint64_t* roff, uint64_t nr,
                              const kmx_window_options* options, kmx_result** out);
kmx_status kmx_search_windows_device(const kmx_index* index, const void* d_ranks, const void* d_roff, uint64_t nr,
                                     const kmx_window_options* options, void* stream, kmx_result** inout);
kmx_status kmx_result_window_offsets(kmx_result* r, const uint64_t** win_off, const uint64_t** d_win_off, uint64_t* nr);

/* ---- seed voting: the candidate loci of every read, from the hit lists of a windows search (an extension, no reference
 *      interface; a caller detects the capability by the macro KMX_WINDOWS_VOTE, KMX_VERSION is unchanged).  What a read mapper,
 *      containment and classification want of kmx_search_windows is not every hit but the places in the text where many windows
 *      of a read agree: the diagonals p - o (text offset minus window offset in the read) that collect votes.  The reduction from
 *      hits to loci runs on the device, on the hit lists where they lie; a few dozen bytes per read cross to the host.
 *
 *      `windows` is the result of the last kmx_search_windows or kmx_search_windows_device into that handle (the handle remembers
 *      that search's w and stride).  For read r with windows j = 0 .. c_r - 1 at read offsets o = j * stride:
 *        - a window VOTES if its status is KMX_Q_OK, it has at least one hit and (max_occ == 0 or its hit count <= max_occ); a
 *          window with hits that fails the max_occ test is counted in skipped[r]; windows without hits and KMX_Q_BAD_RANK windows
 *          (they have no hits) are neither voting nor skipped;
 *        - every hit p of a voting window is one vote on the diagonal D = (int64)p - o.  D is negative when the read would overhang
 *          the start of the text, and D + len_r > n when it overhangs the end: both are reported, never clamped;
 *        - the read's votes are sorted by D; a LOCUS is a maximal run in which each D is at most `band` above the one before it.  It
 *          has diag = its smallest D, span = largest - smallest D (saturated at 2^32 - 1, which only a read of about 2^32 letters
 *          can reach) and votes = the number of votes in it;
 *        - the loci with votes >= min_votes are reported per read in ascending diag: locus_off[nr + 1] is the exclusive prefix sum
 *          of the per-read counts, diag[n_loci] (int64), span[n_loci], votes[n_loci], skipped[nr];
 *        - n_votes is the number of votes cast over the batch; n_small / n_large count the reads by the code path that served
 *          them (a read whose votes fit one workgroup's LDS and whose diagonals fit 32 bits is small; KMX_VOTE_SMALL_CAP in the
 *          environment, read at every call, lowers the cap on the votes, 0 sends every read to the large class); reads that cast
 *          no vote are in neither.  Results never depend on the class.
 *      tests/vote_naive.py is this contract in executable form.
 *
 *      The call runs on the stream of the windows search: the result's own for the host form, the caller's for the device form.
 *      It only reads the result: the views of `windows` are unchanged afterwards and it can be voted on again with other options.
 *      The loci handle owns its buffers, so the result may be searched into again as soon as the call returns.  *inout == NULL
 *      allocates; a handle from an earlier call is reused and its earlier views end.  The device arrays (kmx_loci_view_device;
 *      diag / span / votes are NULL when there is no locus) are complete in stream order when the call returns; kmx_loci_view
 *      copies to page-locked host memory on first use and synchronises.  The votes of over-frequent windows are never
 *      materialised.  The kernel statistics (k_vote) are collected while the index of the search exists.
 *
 *      Refused with KMX_ERR_INVALID_ARGUMENT before the result handle is looked at: a NULL windows, options or inout, a
 *      struct_size that is too small, flags != 0, min_votes == 0.  Refused after looking at the handle: a result that is not
 *      from a windows call or has been searched into by an ordinary search since, a KMX_SEARCH_COUNT_ONLY result (it has no
 *      positions), a result of several parts.  KMX_ERR_TOO_LARGE: a read with 2^32 or more votes, 2^31 or more reads, a read
 *      number and diagonal that do not fit a 64-bit sort key together.  KMX_ERR_OUT_OF_MEMORY when the buffers do not fit: the
 *      caller splits the reads, as for kmx_search_windows.  After a refusal or an error the loci handle, when there is one,
 *      holds an empty result.  The accessors refuse a NULL handle; any of their output pointers may be NULL. */
#define KMX_WINDOWS_VOTE 1
typedef struct kmx_vote_options {
    uint32_t struct_size;  /* = sizeof(kmx_vote_options) */
    uint32_t band;         /* diagonals at most this far from their sorted neighbour join one locus; 0 = exact diagonals */
    uint32_t min_votes;    /* >= 1: loci with fewer votes are not reported */
    uint32_t max_occ;      /* 0 = none; else a window with more than this many hits casts no vote (repeat filter) */
    uint32_t flags;        /* 0 */
} kmx_vote_options;
typedef struct kmx_loci kmx_loci;
kmx_status kmx_windows_vote(kmx_result* windows, const kmx_vote_options* options, kmx_loci** inout);
kmx_status kmx_loci_counts(const kmx_loci* l, uint64_t* nr, uint64_t* n_loci, uint64_t* n_votes,
                           uint64_t* n_small, uint64_t* n_large);
kmx_status kmx_loci_view(kmx_loci* l, const uint64_t** locus_off, const int64_t** diag, const uint32_t** span,
                         const uint32_t** votes, const uint32_t** skipped);
kmx_status kmx_loci_view_device(const kmx_loci* l, const uint64_t** d_locus_off, const int64_t** d_diag,
                                const uint32_t** d_span, const uint32_t** d_votes, const uint32_t** d_skipped);
void kmx_loci_free(kmx_loci* l);

/* ---- alignment at the voted loci: every read against the text around each of its loci (an extension, no reference
 *      interface; a caller detects the capability by the macro KMX_LOCI_ALIGN, KMX_VERSION is unchanged).  It joins the seeds
 *      (kmx_search_windows, kmx_windows_vote) to a verified placement: reads in, (distance, start, end) per locus out, nine
 *      bytes per locus and eight per read to the host.  The edit scripts are a call of their own: kmx_alignments_scripts.
 *
 *      The contract.  ranks / roff[nr + 1] are the reads that were given to the windows search; nr must equal the loci
 *      handle's.  For locus l of read r let q be the read, of m letters, D = diag[l], S = span[l], E = max_edits, n the text
 *      length; all arithmetic in int64:
 *        - S > max_span or m > KMX_ALIGN_MAX_READ: dist[l] = KMX_ALIGN_SKIPPED, start[l] = end[l] = 0;
 *        - otherwise lo = max(0, D - E), hi = max(lo, min(n, D + S + m + E)), T = text[lo, hi) and d = the least Levenshtein
 *          distance (unit costs) between q and any substring of T, the empty one included: the read end to end, the text free
 *          at both ends, no band inside T.  A read letter >= sigma equals no text letter (there is no status for it);
 *        - d > E: dist[l] = KMX_ALIGN_NONE, start[l] = end[l] = 0;
 *        - else dist[l] = d, end[l] = the smallest offset e in [lo, hi] at which a substring of T at distance d ends, start[l] =
 *          the largest s in [lo, e] with lev(q, text[s, e)) == d.  A read that overhangs the text comes out with the overhang
 *          deleted: start = 0 or end = n;
 *        - dist / start / end [n_loci] are parallel to the loci arrays; aligned[nr] = the loci of the read with dist <= E;
 *          best[nr] = the index, relative to locus_off[r], of the aligned locus with the least (dist, index), 0xFFFFFFFF when
 *          the read has none.  Nothing is deduplicated: two loci of a read whose windows overlap may report the same alignment.
 *          n_aligned / n_skipped are the batch totals.
 *      tests/align_naive.py is this contract in executable form.
 *
 *      The handle cannot check that the reads are those of the loci: every access is bounded by roff, n and the loci count
 *      alone, so foreign reads give meaningless but harmless results (the letters [roff[r], roff[r + 1]) must be readable; the
 *      host form refuses a roff that does not start at 0 or decreases, and NULL ranks with roff[nr] != 0).
 *
 *      kmx_loci_align uploads the reads on the stream of the vote that filled the loci handle; kmx_loci_align_device runs on
 *      `stream`, which must be that stream or one the caller has ordered behind it.  The call only reads the loci handle.  The
 *      device arrays (kmx_alignments_view_device; dist / start / end are NULL when there is no locus) are complete in stream
 *      order when the call returns; kmx_alignments_view copies to page-locked host memory on first use and synchronises, on
 *      the stream of the call that filled the handle: after kmx_loci_align_device the caller's stream must still exist at the
 *      first kmx_alignments_view (as for kmx_loci_view after a vote on a device-form result).
 *      *inout == NULL allocates; a handle from an earlier call is reused and its earlier views end.  After a refusal or an error
 *      the handle, when there is one, holds an empty result.  Accessors refuse a NULL handle; any output pointer may be NULL.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: NULL index, loci, options or inout, NULL roff, a struct_size
 *      that is too small, flags != 0, max_edits > KMX_ALIGN_MAX_EDITS.  After looking at the handles: nr differs from the loci's,
 *      the loci live on a device that holds no replica of the index, an index that kmx_index_extend_query_size_range broke
 *      (KMX_ERR_HIP), 2^32 or more loci (KMX_ERR_TOO_LARGE).
 *
 *      kmx_stats_get is not extended: all KMX_N_KERNELS slots are taken and the size of that array is ABI, so the k_align_*
 *      kernels are not timed by the index; tools/probe_align.py times the call from outside. */
#define KMX_LOCI_ALIGN 1
#define KMX_ALIGN_MAX_EDITS 250u
#define KMX_ALIGN_MAX_READ  1024u
#define KMX_ALIGN_SKIPPED   254u
#define KMX_ALIGN_NONE      255u
typedef struct kmx_align_options {
    uint32_t struct_size;  /* = sizeof(kmx_align_options): 16 */
    uint32_t max_edits;    /* E <= KMX_ALIGN_MAX_EDITS */
    uint32_t max_span;     /* loci with span > max_span are not aligned (KMX_ALIGN_SKIPPED); 0 = exact diagonals only */
    uint32_t flags;        /* 0 */
} kmx_align_options;
typedef struct kmx_alignments kmx_alignments;
kmx_status kmx_loci_align(const kmx_index* index, const kmx_loci* loci, const uint8_t* ranks, const uint64_t* roff, uint64_t nr,
                          const kmx_align_options* options, kmx_alignments** inout);
kmx_status kmx_loci_align_device(const kmx_index* index, const kmx_loci* loci, const void* d_ranks, const void* d_roff,
                                 uint64_t nr, const kmx_align_options* options, void* stream, kmx_alignments** inout);
kmx_status kmx_alignments_counts(const kmx_alignments* a, uint64_t* nr, uint64_t* n_loci, uint64_t* n_aligned,
                                 uint64_t* n_skipped);
kmx_status kmx_alignments_view(kmx_alignments* a, const uint8_t** dist, const uint32_t** start, const uint32_t** end,
                               const uint32_t** best, const uint32_t** aligned);
kmx_status kmx_alignments_view_device(const kmx_alignments* a, const uint8_t** d_dist, const uint32_t** d_start,
                                      const uint32_t** d_end, const uint32_t** d_best, const uint32_t** d_aligned);
void kmx_alignments_free(kmx_alignments* a);

/* ---- edit scripts of the alignments: the CIGAR of every read's best alignment, or of every aligned locus (an extension, no
 *      reference interface; a caller detects the capability by the macro KMX_ALIGN_SCRIPTS, KMX_VERSION is unchanged).  It
 *      turns (dist, start, end) into the column-by-column alignment a SAM/BAM record, a pile-up or a variant caller needs,
 *      on the device, from what kmx_loci_align left there.
 *
 *      Selection.  ranks / roff[nr + 1] are the reads that were given to kmx_loci_align.  Locus l of read r is selected when
 *      best[r] != 0xFFFFFFFF and l == locus_off[r] + best[r]; with KMX_SCRIPT_ALL when dist[l] < KMX_ALIGN_SKIPPED.  sel[n_sel]
 *      holds the selected loci as indices into the loci arrays, ascending; read_sel_off[nr + 1] is the exclusive prefix sum of
 *      the per-read counts: the entries of read r are sel[read_sel_off[r] .. read_sel_off[r + 1]).
 *
 *      The script of an entry.  q is the read (m letters), t = text[start[l], end[l]) (L letters); a read letter >= sigma
 *      equals nothing.  H[i][j] is the unit-cost Levenshtein distance of q[0, i) and t[0, j), both ends anchored: H[0][j] = j,
 *      H[i][0] = i.  The script is read off by walking from (m, L) to (0, 0); at (i, j) the first of these that applies:
 *        1. i > 0, j > 0 and H[i-1][j-1] + c == H[i][j] with c = 0 if q[i-1] == t[j-1], else 1: the op is '=' when c == 0 and
 *           'X' when c == 1; go to (i-1, j-1);
 *        2. j > 0 and H[i][j-1] + 1 == H[i][j]: 'D' (a text letter the read lacks); go to (i, j-1);
 *        3. otherwise 'I' (a read letter the text lacks); go to (i-1, j).
 *      The ops in forward order are run-length encoded the BAM way: cigar[x] = len << 4 | op with I = 1, D = 2, '=' = 7,
 *      X = 8; with KMX_SCRIPT_M '=' and 'X' both become M = 0 before the runs are formed.  cig_off[n_sel + 1] delimits the
 *      runs of each entry; n_ops = cig_off[n_sel].  So gaps come out left-aligned, the lengths of X + I + D sum to dist[l],
 *      those of '=' X I to m and those of '=' X D to L, and a script has at most 2 * dist[l] + 1 runs.
 *      tests/script_naive.py is this contract in executable form.
 *
 *      The handle cannot check that the reads are those of the alignment: every access is bounded by roff, n,
 *      m <= KMX_ALIGN_MAX_READ, L <= m + dist and the run reservation alone.  An entry whose read is longer than
 *      KMX_ALIGN_MAX_READ, or with |m - L| > dist[l], or whose DP ends at another distance than dist[l], gets an empty script
 *      and is counted in n_mismatched; with the right reads n_mismatched is 0.  (The letters [roff[r], roff[r + 1]) must be
 *      readable; the host form refuses a roff that does not start at 0 or decreases, and NULL ranks with roff[nr] != 0.)
 *
 *      scratch_bytes bounds the device memory that holds the traceback state (two bits per cell of the band, in rows of 64
 *      diagonals); 0 = 256 MiB.  It is clamped up to what the largest entry of the batch needs, and the entries are processed in
 *      as many chunks as it takes: the result never depends on it.
 *
 *      kmx_alignments_scripts uploads the reads on the stream of the call that filled the alignments handle;
 *      kmx_alignments_scripts_device runs on `stream`, which must be that stream or one the caller has ordered behind it.  The
 *      call only reads the loci and the alignments handle.  The device arrays (kmx_scripts_view_device; sel is NULL when there is
 *      no entry, cigar when there is no run, all four after a refusal or an error) are complete in stream order when the call
 *      returns; kmx_scripts_view copies to page-locked host memory on first use and synchronises, on the stream of the call that
 *      filled the handle: after kmx_alignments_scripts_device the caller's stream must still exist at the first
 *      kmx_scripts_view.
 *      *inout == NULL allocates; a handle from an earlier call is reused and its earlier views end.  After a refusal or an error
 *      the handle, when there is one, holds an empty result.  Accessors refuse a NULL handle; any output pointer may be NULL.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: NULL index, loci, alignments, options or inout, NULL roff, a
 *      struct_size that is too small, a flag bit other than the two.  After looking at the handles: nr differs from the loci's
 *      or the alignments', the alignments' n_loci differs from the loci's, the two handles live on different devices, the loci
 *      live on a device that holds no replica of the index, an index that kmx_index_extend_query_size_range broke
 *      (KMX_ERR_HIP).  KMX_ERR_OUT_OF_MEMORY when the buffers do not fit.
 *
 *      kmx_stats_get is not extended (see kmx_loci_align); tools/probe_script.py times the call from outside. */
#define KMX_ALIGN_SCRIPTS 1
#define KMX_SCRIPT_ALL 1u   /* every aligned locus, not only the best one of each read */
#define KMX_SCRIPT_M   2u   /* '=' and 'X' both reported as M, neighbouring runs joined */
typedef struct kmx_script_options {
    uint32_t struct_size;    /* = sizeof(kmx_script_options): 16 */
    uint32_t flags;          /* 0 or any of the two bits above */
    uint64_t scratch_bytes;  /* cap on the device scratch of the traceback; 0 = the default */
} kmx_script_options;
typedef struct kmx_scripts kmx_scripts;
kmx_status kmx_alignments_scripts(const kmx_index* index, const kmx_loci* loci, const kmx_alignments* alignments,
                                  const uint8_t* ranks, const uint64_t* roff, uint64_t nr, const kmx_script_options* options,
                                  kmx_scripts** inout);
kmx_status kmx_alignments_scripts_device(const kmx_index* index, const kmx_loci* loci, const kmx_alignments* alignments,
                                         const void* d_ranks, const void* d_roff, uint64_t nr,
                                         const kmx_script_options* options, void* stream, kmx_scripts** inout);
kmx_status kmx_scripts_counts(const kmx_scripts* s, uint64_t* nr, uint64_t* n_sel, uint64_t* n_ops, uint64_t* n_mismatched);
kmx_status kmx_scripts_view(kmx_scripts* s, const uint64_t** read_sel_off, const uint32_t** sel, const uint64_t** cig_off,
                            const uint32_t** cigar);
kmx_status kmx_scripts_view_device(const kmx_scripts* s, const uint64_t** d_read_sel_off, const uint32_t** d_sel,
                                   const uint64_t** d_cig_off, const uint32_t** d_cigar);
void kmx_scripts_free(kmx_scripts* s);

/* ---- both strands of the mapping chain: the reverse complements made on the device, the two strands of every read folded into
 *      one placement (an extension, no reference interface; a caller detects the capability by the macro KMX_MAP_STRANDS,
 *      KMX_VERSION is unchanged).  The reverse complement of a read is just another read, and an alignment of rc(read) against
 *      the forward text is what SAM reports for a reverse-strand read: the leftmost forward-text position and the CIGAR of the
 *      reverse-complemented read.  So the four stages stay as they are: the reads go up once, a doubled batch is made on the
 *      device and handed to kmx_search_windows_device, kmx_windows_vote, kmx_loci_align_device; kmx_alignments_fold_strands
 *      picks one placement per read, and kmx_placements_scripts makes the scripts of the winners only.
 *
 *      The doubled batch.  `complement` is the table of kmx_search_approx_strands (sigma entries on the host, an involution on
 *      [0, sigma), the identity allowed; NULL, a non-involution or an entry >= sigma: KMX_ERR_INVALID_ARGUMENT before any device
 *      is touched).  For read i of m letters at roff[i], rc(q)[j] = complement[c] if c < sigma, else c, with c = q[m - 1 - j]: a
 *      letter outside the alphabet stays outside it and matches nothing on either strand.  The internal batch has nr2 = 2 nr
 *      reads: internal read 2i is read i, internal read 2i + 1 is rc(read i), their letters side by side:
 *      roff2[2i] = 2 roff[i], roff2[2i + 1] = 2 roff[i] + m, roff2[2 nr] = 2 roff[nr].
 *      kmx_reads_strands uploads ranks / roff[nr + 1] (shaped as for kmx_search_windows) once, on a stream the handle owns, on
 *      the first replica; it refuses a roff that does not start at 0 or decreases and NULL ranks with roff[nr] != 0.
 *      kmx_reads_strands_device takes device arrays, runs on `stream` on the replica of the device that owns d_ranks (as
 *      kmx_search_windows_device) and costs one 8-byte read-back; reads whose offsets decrease or pass roff[nr] come out empty.
 *      kmx_strand_reads_view_device gives d_ranks2 / d_roff2 / nr2 and the stream the handle was filled on: these four go to
 *      kmx_search_windows_device, kmx_loci_align_device and kmx_alignments_scripts_device as they are (kmx_windows_vote runs on
 *      the stream of its search).  After kmx_reads_strands the handle OWNS that stream: free it after the last *_view of
 *      anything computed on it (the rule written under kmx_loci_align_device, with the handle as the caller).
 *      nr >= 2^30 or more than 2^62 letters: KMX_ERR_TOO_LARGE.  *inout == NULL allocates; a handle passed in is reused and its
 *      earlier views end; after a refusal or an error it holds an empty batch (nr2 = 0).
 *
 *      The fold.  `loci` and `alignments` are those of a doubled batch (nr2 reads, nr2 even; nr = nr2 / 2 public reads); the
 *      reads are not needed.  `stream` is the stream of the align call or one ordered behind it, NULL: the stream that filled
 *      the alignments handle.  For public read i, in int64: a = locus_off[2i], b = locus_off[2i + 1], c = locus_off[2i + 2];
 *      locus l in [a, c) has strand s(l) = 0 if l < b, else 1, and is ALIGNED when dist[l] < KMX_ALIGN_SKIPPED.
 *        - the winner w is the aligned locus with the least (dist, strand, l): the better of a + best[2i] and b + best[2i + 1],
 *          the forward strand winning a tie;
 *        - locus[i] = w (an index into the loci arrays), strand[i] = s(w), dist[i] / start[i] / end[i] those of w; a read without
 *          an aligned locus gets 0xFFFFFFFF, 255, KMX_ALIGN_NONE, 0, 0;
 *        - second[i] = the least dist[l] over the aligned l in [a, c), l != w, that lie ELSEWHERE: s(l) != s(w), or
 *          max(start[l], start[w]) >= min(end[l], end[w]) (no text letter shared with the winner's interval); 255 when there is
 *          none or the read is unplaced.  Two loci of a read often describe one placement (nothing is deduplicated, and a
 *          truncated window yields a worse shadow of the same place): the overlap rule keeps both out of `second`.  A read equal
 *          to its own reverse complement gets second == dist: its strand is ambiguous;
 *        - best2[nr2] is best[] with the loser's entry cleared: best2[2i + s] = best[2i + s] if s == strand[i], else 0xFFFFFFFF;
 *        - n_placed counts the reads with a winner, n_reverse those of them with strand 1, n_ambiguous the placed reads with
 *          second == dist.
 *      tests/fold_naive.py is this contract in executable form.
 *      Every index is bounded by n_loci and every best[] by its read's range: foreign handles give meaningless but harmless
 *      results.  The call only reads the two handles.  The device arrays (kmx_placements_view_device; all NULL when nr == 0)
 *      are complete in stream order when the call returns; kmx_placements_view copies to page-locked host memory on first use
 *      and synchronises, on the stream of the fold (15 bytes per read; best2 only when it is asked for).  *inout and the
 *      accessors as for the other handles; after a refusal or an error the handle holds an empty result.
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: NULL loci, alignments, options or inout, a struct_size that is
 *      too small, flags != 0.  After looking: nr2 odd, the two handles disagree in nr or n_loci or live on different devices.
 *
 *      Scripts of the winners.  kmx_placements_scripts is kmx_alignments_scripts_device over the doubled reads of `reads`, on
 *      the stream that handle was filled on, with the placements' best2 in the place of the alignments' best.  The result is an
 *      ordinary kmx_scripts: read_sel_off[nr2 + 1] runs over the internal reads, with at most one entry per public read, at
 *      internal read 2i + strand[i] and with sel = locus[i]; for a reverse placement the CIGAR is the script of rc(read i)
 *      against text[start, end), the SAM convention.  KMX_SCRIPT_ALL is refused (it ignores best); KMX_SCRIPT_M and
 *      scratch_bytes work as before.  Refused like kmx_alignments_scripts_device, and: NULL reads or placements, placements
 *      whose 2 nr differs from the reads' nr2 or that live on another device. */
#define KMX_MAP_STRANDS 1
typedef struct kmx_strand_reads kmx_strand_reads;
kmx_status kmx_reads_strands(const kmx_index* index, const uint8_t* ranks, const uint64_t* roff, uint64_t nr,
                             const uint8_t* complement, kmx_strand_reads** inout);
kmx_status kmx_reads_strands_device(const kmx_index* index, const void* d_ranks, const void* d_roff, uint64_t nr,
                                    const uint8_t* complement /* host, sigma entries */, void* stream,
                                    kmx_strand_reads** inout);
kmx_status kmx_strand_reads_view_device(const kmx_strand_reads* s, const uint8_t** d_ranks2, const uint64_t** d_roff2,
                                        uint64_t* nr2, void** stream);
void kmx_strand_reads_free(kmx_strand_reads* s);
typedef struct kmx_fold_options {
    uint32_t struct_size;  /* = sizeof(kmx_fold_options): 8 */
    uint32_t flags;        /* 0 */
} kmx_fold_options;
typedef struct kmx_placements kmx_placements;
kmx_status kmx_alignments_fold_strands(const kmx_loci* loci, const kmx_alignments* alignments,
                                       const kmx_fold_options* options, void* stream, kmx_placements** inout);
kmx_status kmx_placements_counts(const kmx_placements* p, uint64_t* nr, uint64_t* n_placed, uint64_t* n_reverse,
                                 uint64_t* n_ambiguous);
kmx_status kmx_placements_view(kmx_placements* p, const uint32_t** locus, const uint8_t** strand, const uint8_t** dist,
                               const uint32_t** start, const uint32_t** end, const uint8_t** second,
                               const uint32_t** best2);
kmx_status kmx_placements_view_device(const kmx_placements* p, const uint32_t** d_locus, const uint8_t** d_strand,
                                      const uint8_t** d_dist, const uint32_t** d_start, const uint32_t** d_end,
                                      const uint8_t** d_second, const uint32_t** d_best2);
void kmx_placements_free(kmx_placements* p);
kmx_status kmx_placements_scripts(const kmx_index* index, const kmx_strand_reads* reads, const kmx_loci* loci,
                                  const kmx_alignments* alignments, const kmx_placements* placements,
                                  const kmx_script_options* options, kmx_scripts** inout);

/* ---- paired-end reads: the two mates of every pair folded into one concordant pair of loci (an extension, no reference
 *      interface; a caller detects the capability by the macro KMX_MAP_PAIRS, KMX_VERSION is unchanged).  Each mate placed on
 *      its own falls to the leftmost copy of a repeat even when its partner sits uniquely a few hundred letters from another
 *      copy; the pair fold picks the two loci together, on the device, from what kmx_loci_align_device left there.
 *
 *      Input.  `loci` and `alignments` are those of a doubled batch (kmx_reads_strands, then the windows search, the vote and the
 *      alignment on d_ranks2 / d_roff2) whose public reads are interleaved mates: public read 2p is mate 1 of pair p, public
 *      read 2p + 1 its mate 2.  nr2 is a multiple of 4 and np = nr2 / 4; internal reads 4p .. 4p + 3 are mate 1 forward, mate 1
 *      reverse complement, mate 2 forward, mate 2 reverse complement.  The reads are not needed.  `stream` as for
 *      kmx_alignments_fold_strands (NULL: the stream that filled the alignments handle).
 *
 *      The contract, in int64.  Locus l of public read i has strand s(l), is ALIGNED and lies ELSEWHERE from another locus of
 *      the same read exactly as kmx_alignments_fold_strands defines them (a locus does not lie elsewhere from itself); single(i)
 *      is that call's winner for read i, the least (dist, strand, l).  For x an aligned locus of mate 1 and y one of mate 2 the
 *      orientation names the upstream locus u and the downstream locus v:
 *        - KMX_PAIR_FR: s(x) != s(y), u the one on strand 0, v the one on strand 1;
 *        - KMX_PAIR_RF: s(x) != s(y), u the one on strand 1, v the one on strand 0;
 *        - KMX_PAIR_FF: s(x) == s(y), u = x and v = y on strand 0, u = y and v = x on strand 1;
 *      loci whose strands do not fit the orientation are never concordant.  With T = end[v] - start[u], (x, y) is CONCORDANT
 *      when start[u] <= start[v], end[u] <= end[v] and min_insert <= T <= max_insert: containment that ends flush is allowed, a
 *      dovetail (start[v] < start[u]) is not.  Its score is dist[x] + dist[y].
 *        - the candidate is the concordant (x, y) with the least (score, x, y), x and y as indices into the loci arrays.  It is
 *          taken when score <= dist[single(mate 1)] + dist[single(mate 2)] + unpaired_penalty (compared without overflow;
 *          0xFFFFFFFF: a concordant pair always wins);
 *        - taken: cls[p] = KMX_PAIR_CONCORDANT, score[p] its score, tlen[p] = +T if u is mate 1, else -T (mate 1's SAM TLEN;
 *          mate 2's is its negative).  second_score[p] = the least score over the concordant (x', y') in which x' lies
 *          elsewhere from x or y' lies elsewhere from y (one of the two at least is not the winner's place on the winner's
 *          strand), 0xFFFF when there is none; the pair counts in n_ambiguous when second_score == score;
 *        - not taken: every mate keeps single().  cls[p] = KMX_PAIR_DISCORDANT, _MATE1_ONLY, _MATE2_ONLY or _UNPLACED by which
 *          mates have an aligned locus, tlen[p] = 0, score[p] = the sum of the placed mates' dist (0xFFFF for UNPLACED),
 *          second_score[p] = 0xFFFF; n_single counts both ONLY classes.
 *      The placements handle is filled for the nr = 2 np public reads in the layout of kmx_alignments_fold_strands: locus /
 *      strand / dist / start / end are those of the chosen locus (x, y, or single(i)), second[i] is that fold's rule with the
 *      chosen locus as w, best2[2i + s] = the chosen locus - locus_off[2i + s] on its strand s and 0xFFFFFFFF on the other, and
 *      n_placed / n_reverse / n_ambiguous follow from these.  kmx_placements_view, _view_device, _counts and
 *      kmx_placements_scripts work on it unchanged (best2 may name a locus that is not the read's best; the scripts only need
 *      it aligned).  For every read of a pair that is not concordant the entries are byte for byte those of
 *      kmx_alignments_fold_strands.  tests/pair_naive.py is this contract in executable form.
 *      Every index is bounded by n_loci and the read's range: foreign handles give meaningless but harmless results.  The call
 *      only reads the loci and the alignments.
 *
 *      The device arrays (kmx_pairs_view_device: cls u8, tlen i32, score u16, second_score u16, one entry per pair; all NULL
 *      when np == 0) are complete in stream order when the call returns; kmx_pairs_view copies 9 bytes per pair to page-locked
 *      host memory on first use and synchronises, on the stream of the fold.  *inout_placements / *inout_pairs == NULL
 *      allocate; a handle passed in is reused and its earlier views end.
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at (both results stay as they were): NULL loci, alignments or
 *      options, NULL for either inout, a struct_size that is too small, flags != 0, orientation > 2, min_insert > max_insert,
 *      max_insert >= 2^31.  After looking (both handles, where they exist, hold an empty result, as after an error): the two
 *      handles disagree in nr or n_loci or live on different devices, nr2 is no multiple of 4. */
#define KMX_MAP_PAIRS 1
#define KMX_PAIR_FR 0u   /* mates face each other: the forward-strand mate is upstream (Illumina paired-end) */
#define KMX_PAIR_RF 1u   /* mates face away: the reverse-strand mate is upstream (mate-pair libraries)       */
#define KMX_PAIR_FF 2u   /* same strand, mate 1 upstream on the forward strand, mate 2 upstream on the reverse */
#define KMX_PAIR_UNPLACED   0u
#define KMX_PAIR_CONCORDANT 1u
#define KMX_PAIR_DISCORDANT 2u   /* both mates placed, each by the single-read rule */
#define KMX_PAIR_MATE1_ONLY 3u
#define KMX_PAIR_MATE2_ONLY 4u
typedef struct kmx_pair_options {
    uint32_t struct_size;       /* = sizeof(kmx_pair_options): 24 */
    uint32_t min_insert;        /* least template length T */
    uint32_t max_insert;        /* greatest T; min_insert <= max_insert < 2^31 */
    uint32_t orientation;       /* KMX_PAIR_FR / _RF / _FF */
    uint32_t unpaired_penalty;  /* see above; 0xFFFFFFFF = a concordant pair always wins */
    uint32_t flags;             /* 0 */
} kmx_pair_options;
typedef struct kmx_pairs kmx_pairs;
kmx_status kmx_alignments_fold_pairs(const kmx_loci* loci, const kmx_alignments* alignments,
                                     const kmx_pair_options* options, void* stream, kmx_placements** inout_placements,
                                     kmx_pairs** inout_pairs);
kmx_status kmx_pairs_counts(const kmx_pairs* p, uint64_t* np, uint64_t* n_concordant, uint64_t* n_discordant,
                            uint64_t* n_single, uint64_t* n_unplaced, uint64_t* n_ambiguous);
kmx_status kmx_pairs_view(kmx_pairs* p, const uint8_t** cls, const int32_t** tlen, const uint16_t** score,
                          const uint16_t** second_score);
kmx_status kmx_pairs_view_device(const kmx_pairs* p, const uint8_t** d_cls, const int32_t** d_tlen,
                                 const uint16_t** d_score, const uint16_t** d_second_score);
void kmx_pairs_free(kmx_pairs* p);

/* ---- mate rescue: an unplaced mate aligned in the insert window of its placed partner (an extension, no reference interface; a
 *      caller detects the capability by the macro KMX_PAIR_RESCUE, KMX_VERSION is unchanged).  kmx_alignments_fold_pairs can
 *      only choose among loci that the seeds voted for: a mate in which sequencing errors or variants leave no intact
 *      w-letter window has none, and its pair comes out KMX_PAIR_MATE1_ONLY / _MATE2_ONLY although the partner pins it to a
 *      few hundred letters of text (or DISCORDANT with a wrong placement, when the mate has an exact copy elsewhere).  The
 *      rescue aligns such a mate against the window that the partner implies, without seeds, and rewrites the placements and
 *      the pairs IN PLACE where the result is concordant.
 *
 *      Input.  `reads`, `loci`, `alignments`, `placements` and `pairs` are those of one doubled batch of interleaved mates after
 *      kmx_alignments_fold_pairs (nr2 = 4 np internal reads); `index` is the index that was searched.  The call runs on the
 *      stream the reads handle was filled on (the stream of the chain), reads the reads, the loci and the alignments, and
 *      writes the placements, the pairs and *inout.  min_insert, max_insert and orientation have the meaning of
 *      kmx_pair_options and normally are the values given to the pair fold; E = max_edits.
 *
 *      Jobs, in int64.  Pair p has mates a (the anchor) and b = 1 - a, public reads 2p + a and 2p + b.  A job (p, b) exists
 *      when cls[p] is the ONLY class in which a is the placed mate (MATE1_ONLY: a = 0, MATE2_ONLY: a = 1), or when
 *      cls[p] == KMX_PAIR_DISCORDANT and KMX_RESCUE_DISCORDANT is set, then for both b.  With s_a, S_a, E_a the strand, start
 *      and end of the anchor in the placements handle, the looked-for strand is s_b = 1 - s_a for KMX_PAIR_FR and _RF and
 *      s_b = s_a for _FF, and the anchor is UPSTREAM iff s_a == 0 (FR), s_a == 1 (RF), (a is mate 1) == (s_a == 0) (FF).  The
 *      job's read q is internal read 4p + 2b + s_b, of m letters; its window is [lo, hi) with lo = S_a,
 *      hi = min(n, S_a + max_insert) when the anchor is upstream, and hi = E_a, lo = max(0, E_a - max_insert) when it is
 *      downstream.  Jobs are ordered by internal read, which is the order of (pair, looked-for mate); an internal read has
 *      at most one.  job_off[nr2 + 1] is the exclusive prefix sum of the jobs per internal read, so the job arrays are shaped
 *      like the loci of the doubled batch: read[j] (the internal read), lo[j], hi[j], dist[j], start[j], end[j], status[j].
 *
 *      The alignment of a job is that of kmx_loci_align with the window given:
 *        - m == 0, m > KMX_ALIGN_MAX_READ or m <= E: dist = KMX_ALIGN_SKIPPED, start = end = 0 (a read of at most E letters
 *          aligns with the empty substring anywhere: that places nothing);
 *        - otherwise d = the least Levenshtein distance (unit costs) between q and any substring of text[lo, hi); a read
 *          letter >= sigma equals no text letter.  d > E: dist = KMX_ALIGN_NONE, start = end = 0;
 *        - else dist = d, end = the smallest e in [lo, hi] at which a substring at distance d ends, start = the largest s in
 *          [lo, e] with lev(q, text[s, e)) == d.
 *
 *      Concordance and the choice.  A found job (dist <= E) is CONCORDANT by the test of kmx_alignments_fold_pairs itself,
 *      applied to the anchor's interval and [start, end) with the strands s_a, s_b: start[u] <= start[v], end[u] <= end[v]
 *      and min_insert <= T <= max_insert with T = end[v] - start[u].  (The window guarantees one inequality and the upper
 *      bound; the rest is tested.)  Its score is dist[anchor] + d.  The limit of the method: the best alignment of a window
 *      that is not concordant (the mate inside the anchor's interval, a dovetail, T < min_insert) is NOT replaced by a worse
 *      one that would be.
 *        - an ONLY pair takes its concordant job;
 *        - a DISCORDANT pair takes the concordant job with the least (score, b) when
 *          score <= dist[mate 1] + dist[mate 2] + unpaired_penalty (the placements' distances, compared without overflow;
 *          0xFFFFFFFF: a rescued pair always wins).  unpaired_penalty is not looked at for ONLY pairs;
 *        - status[j] = 0 skipped or none, 1 found but not concordant, 2 concordant but not taken, 3 taken.
 *      A taken job writes, for pair p: cls = KMX_PAIR_CONCORDANT, tlen = +T if the upstream one is mate 1, else -T, score =
 *      the job's score, second_score = 0xFFFF (no runner-up pair is searched for: a rescued pair never counts as ambiguous);
 *      and for public read 2p + b: locus = 0xFFFFFFFF (the placement is no locus: read it from strand / dist / start / end),
 *      strand = s_b, dist / start / end the job's, both best2 entries 0xFFFFFFFF (kmx_placements_scripts has no entry for the
 *      read; kmx_rescues_scripts has), second = the least dist[l] over the ALIGNED loci l of the read that lie ELSEWHERE
 *      from (s_b, [start, end)) by the rule of kmx_alignments_fold_strands: s(l) != s_b, or
 *      max(start[l], start) >= min(end[l], end); 255 when there is none.  The anchor's entries and every other pair stay byte
 *      for byte.  All counters of the two handles (n_placed, n_reverse, n_ambiguous; n_concordant, n_discordant, n_single,
 *      n_unplaced, the pairs' n_ambiguous) are recounted from the final arrays, and the host views of both handles are
 *      taken anew at their next kmx_*_view (earlier host views end).  A second rescue of the same handles with the same
 *      options takes nothing.  tests/rescue_naive.py is this contract in executable form.
 *
 *      `segment` = G only shapes the work: a thread per (job, G end columns), each starting with a fresh state m + E columns
 *      before its own range; 0 = 512.  The result never depends on it.
 *
 *      The rescues handle.  n_jobs, n_found (status >= 1), n_concordant (>= 2), n_taken (== 3) are the batch totals.  The
 *      device arrays (kmx_rescues_view_device; job_off is NULL after a refusal or an error, the job arrays when there is no
 *      job) are complete in stream order when the call returns; kmx_rescues_view copies to page-locked host memory on first
 *      use and synchronises, on the stream of the call.  *inout == NULL allocates; a handle passed in is reused and its
 *      earlier views end.  The placements and the pairs are written by the last kernel only: after a refusal, or an error
 *      before that kernel, they are untouched and the rescues handle, when there is one, holds an empty result; after an
 *      error behind it all three hold an empty result.  Every index is bounded by n, n_loci, nr2 and the job count: foreign
 *      handles give meaningless but harmless results.
 *
 *      kmx_rescues_scripts is kmx_alignments_scripts_device over the doubled reads of `reads` with the job arrays in the place
 *      of the loci and their alignments and only the taken jobs selected.  The result is an ordinary kmx_scripts over the
 *      internal reads: at most one entry per rescued read, at internal read 4p + 2b + s_b, with sel = the job's index; for a
 *      reverse placement the CIGAR is that of the reverse complement against text[start, end), the SAM convention.
 *      KMX_SCRIPT_ALL is refused; KMX_SCRIPT_M and scratch_bytes work as before.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: a NULL argument, a struct_size that is too small, a flag bit
 *      other than KMX_RESCUE_DISCORDANT, orientation > 2, min_insert > max_insert, max_insert > KMX_RESCUE_MAX_INSERT,
 *      max_edits > KMX_ALIGN_MAX_EDITS.  After looking: the handles disagree in nr / nr2 / np / n_loci or live on different
 *      devices, nr2 is no multiple of 4, the device holds no replica of the index, an index that
 *      kmx_index_extend_query_size_range broke (KMX_ERR_HIP).  kmx_stats_get is not extended (see kmx_loci_align). */
#define KMX_PAIR_RESCUE 1
#define KMX_RESCUE_DISCORDANT 1u      /* also try DISCORDANT pairs, both ways round */
#define KMX_RESCUE_MAX_INSERT 65536u
typedef struct kmx_rescue_options {
    uint32_t struct_size;       /* = sizeof(kmx_rescue_options): 32 */
    uint32_t min_insert;        /* as kmx_pair_options */
    uint32_t max_insert;        /* min_insert <= max_insert <= KMX_RESCUE_MAX_INSERT: the columns of a window */
    uint32_t orientation;       /* KMX_PAIR_FR / _RF / _FF */
    uint32_t max_edits;         /* E <= KMX_ALIGN_MAX_EDITS */
    uint32_t unpaired_penalty;  /* only looked at for DISCORDANT pairs; 0xFFFFFFFF = a rescued pair always wins */
    uint32_t segment;           /* end columns per thread of the forward pass; 0 = the default (512) */
    uint32_t flags;             /* 0 or KMX_RESCUE_DISCORDANT */
} kmx_rescue_options;
typedef struct kmx_rescues kmx_rescues;
kmx_status kmx_pairs_rescue(const kmx_index* index, const kmx_strand_reads* reads, const kmx_loci* loci,
                            const kmx_alignments* alignments, const kmx_rescue_options* options, kmx_placements* placements,
                            kmx_pairs* pairs, kmx_rescues** inout);
kmx_status kmx_rescues_counts(const kmx_rescues* r, uint64_t* nr2, uint64_t* n_jobs, uint64_t* n_found, uint64_t* n_concordant,
                              uint64_t* n_taken);
kmx_status kmx_rescues_view(kmx_rescues* r, const uint64_t** job_off, const uint32_t** read, const uint32_t** lo,
                            const uint32_t** hi, const uint8_t** dist, const uint32_t** start, const uint32_t** end,
                            const uint8_t** status);
kmx_status kmx_rescues_view_device(const kmx_rescues* r, const uint64_t** d_job_off, const uint32_t** d_read,
                                   const uint32_t** d_lo, const uint32_t** d_hi, const uint8_t** d_dist, const uint32_t** d_start,
                                   const uint32_t** d_end, const uint8_t** d_status);
kmx_status kmx_rescues_scripts(const kmx_index* index, const kmx_strand_reads* reads, const kmx_rescues* rescues,
                               const kmx_script_options* options, kmx_scripts** inout);
void kmx_rescues_free(kmx_rescues* r);

/* ---- SAM tags: the MD string of every script and a MAPQ per read (an extension, no reference interface; a caller detects the
 *      capability by the macro KMX_SAM_TAGS, KMX_VERSION is unchanged).  The chain gives FLAG, POS, CIGAR, TLEN and NM (= dist)
 *      of a SAM record; these two calls give what was missing, from arrays that are on the device already.  Neither needs the
 *      reads.
 *
 *      MD.  kmx_scripts_md serves the scripts of kmx_alignments_scripts[_device] (KMX_SCRIPT_ALL or not) and of
 *      kmx_placements_scripts: `alignments` is the handle the scripts were made from, sel[e] indexes its start / end, bounded
 *      by n_loci.  kmx_rescues_md serves the scripts of kmx_rescues_scripts: sel[e] indexes the job arrays of `rescues`, bounded
 *      by n_jobs.  `index` is the index that was searched; its packed text (kmx_index_text) is derived on first use.
 *      `letters` is a host table of sigma bytes, rank -> output byte (e.g. "ACGT"); duplicates are allowed.  `stream` NULL means
 *      the stream the scripts handle was filled on, else it is that stream or one the caller has ordered behind it.
 *
 *      The contract of entry e, with l = sel[e], s = start[l], t = end[l], n the text length and the runs
 *      cigar[cig_off[e] .. cig_off[e + 1]): a match counter c = 0 and a text cursor j = s; the runs in order:
 *        '=' of length len: c += len, j += len;
 *        'I': nothing;
 *        'X' of length len: for each letter emit decimal(c), emit letters[text[j]], then c = 0, ++j;
 *        'D' of length len: emit decimal(c), emit '^', emit letters[text[j .. j + len)], then c = 0, j += len;
 *      at the end emit decimal(c).  This is the SAM specification's [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*: it gives 0 between
 *      adjacent mismatches, after a deletion that a mismatch follows, and at either end.  md_off[n_sel + 1] is the exclusive
 *      prefix sum of the byte counts, md the bytes; there are no terminators.  An entry without runs has an empty MD and is
 *      not counted.  An entry gets an empty MD and counts in n_mismatched when l is out of bound, when not s <= t <= n, when
 *      it has an op other than = X I D, or when its = X D lengths do not sum to t - s (or when its MD would take 2^32 bytes or
 *      more).  With the right handles n_mismatched is 0.  Every access is bounded by n_sel, n_ops, the bound on sel and n:
 *      foreign handles give meaningless but harmless results.  tests/md_naive.py is this contract in executable form.
 *
 *      The md handle.  The device arrays (kmx_md_view_device; md_off is NULL after a refusal or an error, md when n_bytes == 0)
 *      are complete in stream order when the call returns; kmx_md_view copies to page-locked host memory on first use and
 *      synchronises, on the stream of the call: 8 bytes per entry and the strings (md_off always holds at least the one
 *      offset 0).  *inout == NULL allocates; a handle passed in is reused and its earlier views end.  The call only reads the
 *      other handles.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at and before any device is touched: a NULL argument, a
 *      struct_size that is too small, flags != 0, a letters table with 0, '^' or a digit among its first sigma entries.  After
 *      looking: a scripts handle made with KMX_SCRIPT_M ('=' and 'X' are no longer apart), handles that live on different
 *      devices, a device without a replica of the index, an index that kmx_index_extend_query_size_range broke (KMX_ERR_HIP).
 *      After such a refusal or an error the md handle, when there is one, holds an empty result.
 *
 *      MAPQ.  A MAPQ is a convention, not a measurement: this one is a GAP RULE, a heuristic that grows with the distance
 *      between the chosen placement and its runner-up, and claims no calibration as a probability.  In int64, with E =
 *      max_edits (the budget the alignments, and the rescue, were made with):
 *        q(d, s, B) = min(cap, per_edit * max(0, s' - d)),   s' = B + 1 when s is "none", else s;
 *        read i unplaced (strand == 255): 0;
 *        otherwise q_se = q(dist[i], second[i], E), where 255 means none;
 *        without `pairs`, or when cls[i / 2] != KMX_PAIR_CONCORDANT: mapq[i] = q_se;
 *        for a concordant pair p = i / 2: q_pe = q(score[p], second_score[p], 2 E), where 0xFFFF means none, and
 *        mapq[i] = min(cap, max(q_se, min(q_pe, q_se + pair_bonus))).
 *      So a read equal to its reverse complement, or with an equal copy elsewhere, gets 0; a mate inside a repeat that followed
 *      its unique partner gets min(cap, pair_bonus).  The limit: a rescued pair has second_score == 0xFFFF (no runner-up pair
 *      is searched for), so it looks unique.  n_zero counts the PLACED reads with mapq 0, n_cap the reads with mapq == cap.
 *      `pairs` NULL: single reads (kmx_alignments_fold_strands).  `stream` NULL means the stream that filled the placements;
 *      a rescue rewrites them on the stream of the chain, so the order holds.  tests/mapq_naive.py is this contract in
 *      executable form.  A placements handle with nr == 0 gives an empty result with all views NULL; kmx_mapq_view copies 1
 *      byte per read.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: NULL placements, options or inout, a struct_size that is too
 *      small, flags != 0, max_edits > KMX_ALIGN_MAX_EDITS, cap > 254.  After looking: pairs with 2 np != nr, or that live on
 *      another device; the mapq handle, when there is one, then holds an empty result.  kmx_stats_get is not extended (see
 *      kmx_loci_align). */
#define KMX_SAM_TAGS 1
typedef struct kmx_md_options {
    uint32_t struct_size;  /* = sizeof(kmx_md_options): 8 */
    uint32_t flags;        /* 0 */
} kmx_md_options;
typedef struct kmx_md kmx_md;
kmx_status kmx_scripts_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_alignments* alignments,
                          const uint8_t* letters, const kmx_md_options* options, void* stream, kmx_md** inout);
kmx_status kmx_rescues_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_rescues* rescues, const uint8_t* letters,
                          const kmx_md_options* options, void* stream, kmx_md** inout);
kmx_status kmx_md_counts(const kmx_md* m, uint64_t* n_sel, uint64_t* n_bytes, uint64_t* n_mismatched);
kmx_status kmx_md_view(kmx_md* m, const uint64_t** md_off /* n_sel + 1 */, const uint8_t** md /* n_bytes */);
kmx_status kmx_md_view_device(const kmx_md* m, const uint64_t** d_md_off, const uint8_t** d_md);
void kmx_md_free(kmx_md* m);
typedef struct kmx_mapq_options {
    uint32_t struct_size;  /* = sizeof(kmx_mapq_options): 24 */
    uint32_t max_edits;    /* E <= KMX_ALIGN_MAX_EDITS: the budget the alignments (and the rescue) were made with */
    uint32_t cap;          /* <= 254 (255 is SAM's "unavailable") */
    uint32_t per_edit;
    uint32_t pair_bonus;
    uint32_t flags;        /* 0 */
} kmx_mapq_options;
typedef struct kmx_mapq kmx_mapq;
kmx_status kmx_placements_mapq(const kmx_placements* placements, const kmx_pairs* pairs /* NULL: single reads */,
                               const kmx_mapq_options* options, void* stream, kmx_mapq** inout);
kmx_status kmx_mapq_counts(const kmx_mapq* m, uint64_t* nr, uint64_t* n_zero, uint64_t* n_cap);
kmx_status kmx_mapq_view(kmx_mapq* m, const uint8_t** mapq /* nr */);
kmx_status kmx_mapq_view_device(const kmx_mapq* m, const uint8_t** d_mapq);
void kmx_mapq_free(kmx_mapq* m);

/* ---- Multi-sequence references: a contig table through the mapping chain (an extension, no reference interface; a caller
 *      detects the capability by the macro KMX_MAP_CONTIGS, KMX_VERSION is unchanged).  A real reference has many sequences
 *      (chromosomes, contigs, transcripts, amplicons); the index text is their concatenation.  With a table on the index the
 *      device stages that choose (alignment window, pair fold, rescue window) keep every alignment, pair and rescue inside one
 *      contig, and kmx_placements_locate turns a placement into (contig, position inside it).  AN INDEX WITHOUT A TABLE BEHAVES
 *      EXACTLY AS BEFORE, IN EVERY CALL.
 *
 *      The table.  kmx_index_set_contigs(index, ctg_off, nc): contig c is text[ctg_off[c], ctg_off[c + 1]), ctg_off is a host
 *      array of nc + 1 offsets that is copied (to every replica of the index).  nc == 0 removes the table (ctg_off is not looked
 *      at).  KMX_ERR_INVALID_ARGUMENT, the table that was there staying in place: a NULL index, NULL ctg_off with nc > 0,
 *      nc >= 0xFFFFFFFF, ctg_off[0] != 0, offsets that are not strictly ascending (an empty contig), ctg_off[nc] != n (the
 *      text length); KMX_ERR_HIP for an index that kmx_index_extend_query_size_range broke.  Every successful call gives the
 *      index a new table GENERATION (a private counter).  It must not be called while a chain call on this index is in flight
 *      on another thread; it synchronises the devices of the index before it frees the previous table, so kernels that were
 *      enqueued earlier have finished reading it.  kmx_index_contigs reads the table back: *nc (0: none) and, when ctg_off_out
 *      is not NULL, the nc + 1 offsets (cap, the room in offsets, must be at least nc + 1).  THE TABLE IS NOT PART OF THE
 *      SAVED IMAGE (kmx_index_save / kmx_index_load are unchanged): a caller sets it again after kmx_index_load.
 *
 *      Alignment.  kmx_loci_align[_device] on an index with a table: for every locus l that is not skipped, in int64 with
 *      D = diag[l], S = span[l], m the read's length, E = max_edits and floor division,
 *        mid  = clamp(D + (S + m) / 2, 0, n - 1),     c(l) = the contig that contains mid,
 *        lo   = min(max(ctg_off[c], D - E), ctg_off[c + 1]),
 *        hi   = max(lo, min(ctg_off[c + 1], D + S + m + E)),
 *      and everything else by the contract of kmx_loci_align over T = text[lo, hi): a read that overhangs the contig's end
 *      comes out with the overhang deleted, exactly as at the ends of the text without a table.  Equivalently: the contract
 *      without a table, applied to the contig's letters alone with diagonal D - ctg_off[c], shifted back by ctg_off[c].  No
 *      aligned [start, end) therefore contains a junction.  The handle keeps c(l) per locus: kmx_alignments_contigs_view and
 *      kmx_alignments_contigs_view_device give ctg[n_loci] (u32; 0xFFFFFFFF for a skipped locus, c(l) for every other one,
 *      KMX_ALIGN_NONE loci included) and *nc, the contigs of the table the call saw; ctg is NULL (and *nc 0) when the handle
 *      was made without a table, and NULL when n_loci == 0.  The host view copies 4 bytes per locus on first use.  The handle
 *      also records the generation of the table.
 *
 *      Pair fold.  kmx_alignments_fold_pairs on alignments that carry ctg: (x, y) is concordant only if ctg[x] == ctg[y] as
 *      well, for the candidate and for second_score alike.  Nothing else changes; the call takes no index.
 *      kmx_alignments_fold_strands is unchanged.
 *
 *      Rescue.  kmx_pairs_rescue: the anchor of a job is placed by a locus, its contig is ctg[locus[anchor]], and the job's
 *      window [lo, hi) is clamped to that contig (ctg_off[c] in the place of 0, ctg_off[c + 1] in the place of n).  A rescued
 *      mate therefore lies in its anchor's contig.  The call is refused after looking at the handles
 *      (KMX_ERR_INVALID_ARGUMENT, the rescues handle then holds an empty result) when the alignments' nc or generation
 *      differs from the index's: a handle made without a table, or under another one.
 *
 *      kmx_placements_locate(index, alignments, placements, options, stream, &located): per public read i of the placements
 *      (of kmx_alignments_fold_strands, of kmx_alignments_fold_pairs, or after a rescue), ctg[i] and pos[i] (u32 each):
 *        unplaced (strand == 255): 0xFFFFFFFF and 0;
 *        placed by a locus: c = alignments.ctg[locus[i]];
 *        rescued (placed, locus == 0xFFFFFFFF): with KMX_LOCATE_MATES in flags (the reads are interleaved mates, nr even)
 *          c = alignments.ctg[locus[i ^ 1]], the mate's;
 *        pos[i] = start[i] - ctg_off[c]   (0-based; SAM's POS is pos + 1).
 *      No search is made, and the answer is exact even for an empty alignment that sits on a junction.  An entry is written
 *      as unplaced and counted in n_mismatched when the locus is outside n_loci, when c >= nc, when start is outside
 *      [ctg_off[c], ctg_off[c + 1]], or when a rescued read comes without the flag or without a mate placed by a locus;
 *      n_located counts the other placed reads.  With the right handles n_mismatched is 0.  Every access is bounded by nr,
 *      n_loci and nc: foreign handles give meaningless but harmless results.  `stream` NULL means the stream that filled the
 *      placements.  The located handle follows the lifecycle of the other chain handles: *inout == NULL allocates, a handle
 *      passed in is reused and its earlier views end; the device arrays (kmx_located_view_device, NULL when nr == 0) are
 *      complete in stream order when the call returns; kmx_located_view copies 8 bytes per read to page-locked host memory
 *      on first use and synchronises.  KMX_ERR_INVALID_ARGUMENT before any handle is looked at: a NULL argument, a
 *      struct_size that is too small, an unknown flag.  After looking (the located handle, when there is one, then holds an
 *      empty result): KMX_LOCATE_MATES with an odd nr, placements whose 2 nr differs from the alignments' nr, handles on
 *      different devices, a device without a replica of the index, a broken index (KMX_ERR_HIP), alignments whose nc or
 *      generation differs from the index's, an index without a table.  tests/contig_naive.py is all of this in executable
 *      form.  Untested: an index with more than one replica.  kmx_stats_get is not extended (see kmx_loci_align). */
#define KMX_MAP_CONTIGS 1
#define KMX_LOCATE_MATES 1u   /* the reads are interleaved mates: a rescued read takes its mate's contig */
kmx_status kmx_index_set_contigs(kmx_index* index, const uint64_t* ctg_off /* nc + 1 */, uint64_t nc);
kmx_status kmx_index_contigs(const kmx_index* index, uint64_t* nc, uint64_t* ctg_off_out, uint64_t cap);
kmx_status kmx_alignments_contigs_view(kmx_alignments* a, const uint32_t** ctg /* n_loci */, uint64_t* nc);
kmx_status kmx_alignments_contigs_view_device(const kmx_alignments* a, const uint32_t** d_ctg, uint64_t* nc);
typedef struct kmx_locate_options {
    uint32_t struct_size;  /* = sizeof(kmx_locate_options): 8 */
    uint32_t flags;        /* 0 or KMX_LOCATE_MATES */
} kmx_locate_options;
typedef struct kmx_located kmx_located;
kmx_status kmx_placements_locate(const kmx_index* index, const kmx_alignments* alignments, const kmx_placements* placements,
                                 const kmx_locate_options* options, void* stream, kmx_located** inout);
kmx_status kmx_located_counts(const kmx_located* l, uint64_t* nr, uint64_t* n_located, uint64_t* n_mismatched);
kmx_status kmx_located_view(kmx_located* l, const uint32_t** ctg /* nr */, const uint32_t** pos /* nr */);
kmx_status kmx_located_view_device(const kmx_located* l, const uint32_t** d_ctg, const uint32_t** d_pos);
void kmx_located_free(kmx_located* l);

/* ---- Secondary placements: up to N further places per read (an extension, no reference interface; a caller detects the
 *      capability by the macro KMX_MAP_SECONDARIES, KMX_VERSION is unchanged).  The folds report one placement per read and one
 *      byte, second, about every other place it fits.  A read from a repeat family, an amplicon panel or a transcriptome fits
 *      in many places, and a caller who writes XA:Z: or quantifies needs them.  Two loci of a read often describe the SAME
 *      place (nothing upstream deduplicates them; a truncated window yields a worse shadow), so the N best loci are not the N
 *      best places: this call applies the fold's ELSEWHERE rule transitively, on the device, and sends 13 bytes per reported
 *      place to the host in the place of 9 per locus.
 *
 *      Input.  `loci` and `alignments` are those of a doubled batch (nr2 internal reads, nr = nr2 / 2 public ones);
 *      `placements` is the handle of kmx_alignments_fold_strands or of kmx_alignments_fold_pairs, before or after
 *      kmx_pairs_rescue: its locus / strand / dist / start / end are read.  The reads and the index are not needed.  `stream`
 *      NULL means the stream that filled the placements; a rescue rewrites them on the stream of the chain, so the order
 *      holds.  A caller who passes another stream orders it behind the stream that filled the placements, and orders the
 *      stream of every later call that reads the secondaries (kmx_secondaries_scripts runs on the stream of `reads`,
 *      kmx_secondaries_md on the scripts' or the one it is given) behind it: the last kernel of this call is left in flight
 *      on `stream`, as with the other stream-taking calls of the chain.  N = max_secondary.
 *
 *      Candidates, in int64.  For public read i: a = locus_off[2i], b = locus_off[2i + 1], c = locus_off[2i + 2], each clamped
 *      into [0, n_loci] and made ascending as the strand fold does; locus l has strand 0 if l < b, else 1.  The primary is
 *      P = (strand[i], start[i], end[i]) of the placements, its distance dist[i].  An unplaced read (strand[i] == 255) has no
 *      entries and more[i] = 0.  A locus l in [a, c) is a CANDIDATE when dist[l] < KMX_ALIGN_SKIPPED, l != locus[i], and
 *      dist[l] <= dist[i] + max_delta (max_delta == 0xFFFFFFFF: always).  Two places (s, x0, x1) and (t, y0, y1) lie ELSEWHERE
 *      from each other when s != t or max(x0, y0) >= min(x1, y1): the rule of kmx_alignments_fold_strands, on intervals.
 *
 *      The greedy selection.  T = {P}.  Repeat: among the candidates not yet taken that lie elsewhere from EVERY member of T,
 *      find the one with the least (dist, l) (a forward locus has the lower index, so this is the fold's (dist, strand, l));
 *      if there is none, stop with more[i] = 0; if N have been taken already, stop with more[i] = 1; otherwise take it and
 *      add (its strand, start[l], end[l]) to T.  A locus that overlaps a taken place stays excluded for good, so a chain of
 *      mutually overlapping loci gives one place.  A rescued read (placed, locus[i] == 0xFFFFFFFF) works the same way: its
 *      primary is the interval in the placements, and no candidate is excluded by index.  With max_delta unbounded and the
 *      placements of the strand fold, the least dist among the entries of a read equals second[i] (255: no entry).
 *
 *      Output.  The taken loci of read i in ASCENDING LOCUS INDEX, forward strand first.  sec_off[nr2 + 1] (u64) counts them
 *      per INTERNAL read: the entries of public read i are [sec_off[2i], sec_off[2i + 2)), those on strand s
 *      [sec_off[2i + s], sec_off[2i + s + 1)), which is the shape the script stage needs.  Per entry e: locus[e] (u32, an
 *      index into the loci arrays), dist[e] (u8), start[e], end[e] (u32) and, when the alignments carry a contig table,
 *      ctg[e] (u32) = the alignments' ctg[locus[e]] (the view is NULL otherwise).  Per public read: more[nr] (u8).  Counters:
 *      n_sec = sec_off[nr2], n_multi = the reads with at least one entry, n_truncated = the reads with more == 1.  Every
 *      index is bounded by n_loci, nr and the read's own range: foreign handles give meaningless but harmless results.
 *      tests/secondary_naive.py is this contract in executable form.
 *
 *      The secondaries handle.  *inout == NULL allocates; a handle passed in is reused and its earlier views end.  The device
 *      arrays (kmx_secondaries_view_device; sec_off is NULL after a refusal or an error, the entry arrays when n_sec == 0,
 *      more when nr == 0) are complete in stream order when the call returns; kmx_secondaries_view copies to page-locked host
 *      memory on first use and synchronises, on the stream of the call: 13 bytes per entry (17 with ctg), 8 per internal
 *      read, 1 per public read (sec_off always holds at least the one offset 0).  Any output pointer may be NULL.  The call
 *      only reads the other handles.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: a NULL argument, a struct_size that is too small, flags != 0,
 *      max_secondary == 0 or > KMX_SECONDARY_MAX.  After looking (the secondaries handle, when there is one, then holds an
 *      empty result): nr2 odd, placements whose 2 nr differs from the alignments' nr, loci and alignments that disagree in nr
 *      or n_loci, handles on different devices; KMX_ERR_TOO_LARGE when nr * N >= 2^32.
 *
 *      CIGAR and MD of the entries.  kmx_secondaries_scripts is kmx_alignments_scripts_device over the doubled reads of
 *      `reads` with the entry arrays in the place of the loci and their alignments and EVERY entry selected: an ordinary
 *      kmx_scripts over the internal reads with sel[e] == e; for a reverse entry the script is that of the reverse complement
 *      against text[start, end), the SAM convention.  It runs on the stream of `reads`.  KMX_SCRIPT_ALL in the options is
 *      refused (there is nothing to add); KMX_SCRIPT_M and scratch_bytes work as before.  Refused after looking: secondaries
 *      whose 2 nr differs from the reads' nr2, or that live on another device, and what kmx_rescues_scripts refuses about the
 *      index.  kmx_secondaries_md is kmx_rescues_md over these scripts: sel[e] indexes start / end of the entries, bounded by
 *      n_sec.  With it a caller can build secondary SAM lines; no call here writes them.  Untested: handles on different
 *      devices.  kmx_stats_get is not extended (see kmx_loci_align). */
#define KMX_MAP_SECONDARIES 1
#define KMX_SECONDARY_MAX 32
typedef struct kmx_secondary_options {
    uint32_t struct_size;    /* = sizeof(kmx_secondary_options): 16 */
    uint32_t max_secondary;  /* N, in 1 .. KMX_SECONDARY_MAX */
    uint32_t max_delta;      /* a candidate has dist <= the primary's + max_delta; 0xFFFFFFFF: no bound */
    uint32_t flags;          /* 0 */
} kmx_secondary_options;
typedef struct kmx_secondaries kmx_secondaries;
kmx_status kmx_placements_secondaries(const kmx_loci* loci, const kmx_alignments* alignments, const kmx_placements* placements,
                                      const kmx_secondary_options* options, void* stream, kmx_secondaries** inout);
kmx_status kmx_secondaries_counts(const kmx_secondaries* s, uint64_t* nr, uint64_t* n_sec, uint64_t* n_multi, uint64_t* n_truncated);
kmx_status kmx_secondaries_view(kmx_secondaries* s, const uint64_t** sec_off /* 2 nr + 1 */, const uint32_t** locus /* n_sec */,
                                const uint8_t** dist, const uint32_t** start, const uint32_t** end, const uint32_t** ctg /* or NULL */,
                                const uint8_t** more /* nr */);
kmx_status kmx_secondaries_view_device(const kmx_secondaries* s, const uint64_t** d_sec_off, const uint32_t** d_locus,
                                       const uint8_t** d_dist, const uint32_t** d_start, const uint32_t** d_end, const uint32_t** d_ctg,
                                       const uint8_t** d_more);
kmx_status kmx_secondaries_scripts(const kmx_index* index, const kmx_strand_reads* reads, const kmx_secondaries* secondaries,
                                   const kmx_script_options* options, kmx_scripts** inout);
kmx_status kmx_secondaries_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_secondaries* secondaries,
                              const uint8_t* letters, const kmx_md_options* options, void* stream, kmx_md** inout);
void kmx_secondaries_free(kmx_secondaries* s);

/* ---- Soft clipping: every script trimmed to its best-scoring part (an extension, no reference interface; a caller detects the
 *      capability by the macro KMX_SOFT_CLIP, KMX_VERSION is unchanged).  The chain aligns every read END TO END at unit cost:
 *      a read that overhangs the end of the text or of a contig comes out with the overhang as a terminal 'I' run, and a read
 *      with an adapter tail or a chimeric end carries a dozen X / I / D at one end, which count in NM, in the MD string and in
 *      XA.  SAM writes such ends as 'S'.  kmx_scripts_clip trims the runs of every entry of a scripts handle under an affine
 *      scoring and gives the score (SAM's AS:i) with it.
 *
 *      THIS IS POST-ALIGNMENT TRIMMING OF THE EDIT-OPTIMAL SCRIPT, NOT A SMITH-WATERMAN REALIGNMENT.  The clipped alignment is
 *      the best-scoring PART OF THE CANONICAL SCRIPT, not the best local alignment of the read: no cell of a dynamic programme
 *      is computed again, and a better local alignment that the unit-cost script does not contain is not found.
 *      kmx_scripts_realign (below, KMX_REALIGN) is the call that computes one, inside the band of the script.
 *
 *      Input.  The call takes ONLY a scripts handle: no index, no reads, no alignments.  It serves the scripts of
 *      kmx_alignments_scripts[_device] (KMX_SCRIPT_ALL or not), kmx_placements_scripts, kmx_rescues_scripts and
 *      kmx_secondaries_scripts alike.  Entry e of the clips is entry e of the scripts.  `stream` NULL means the stream that
 *      filled the scripts, else it is that stream or one the caller has ordered behind it.
 *
 *      The contract of entry e, with the runs r_0 .. r_{R-1} = cigar[cig_off[e] .. cig_off[e + 1]) of the scripts and the
 *      options a = match, b = mismatch, o = gap_open, x = gap_extend, p = clip_penalty, everything in int64:
 *        w('=' of len) = len a,  w('X') = -len b,  w('I') = w('D') = -(o + len x);  W[0] = 0, W[k + 1] = W[k] + w(r_k);
 *        a LEFT CUT i is 0, or any k with r_k an '=' run; a RIGHT CUT j is R, or any k with r_{k-1} an '=' run;
 *        the candidates are all (i, j) with i < j, and (0, R) always, even for R = 0;
 *        V(i, j) = W[j] - W[i] - p [i > 0] - p [j < R];
 *        the candidate with the greatest V is taken; among equals the smallest i, then the largest j;
 *        if that V < min_score the entry stays whole, (i, j) = (0, R), and the bit KMX_CLIP_LOW is set in cflags[e].
 *      Per entry: score[e] (i32) = V of the (i, j) that is kept (for a LOW entry V(0, R) = W[R], the score of what is written),
 *      saturated to the int32 range; sl[e] / sr[e] (u16) = the read letters ('=' 'X' 'I') of the runs in front of i / from j
 *      on; tl[e] / tr[e] (u16) = the text letters ('=' 'X' 'D') of the same runs; nm[e] (u16) = the 'X' + 'I' + 'D' lengths of
 *      the kept runs (the five saturate at 65535, which a script of the chain never reaches); cflags[e] (u8).  The new runs:
 *      sl 'S' (only if sl > 0), r_i .. r_{j-1}, sr 'S' (only if sr > 0); 'S' is BAM op 4; cig_off[n_sel + 1] (u64) delimits
 *      them, n_ops = cig_off[n_sel].  So: a clipped side always borders an '=' run, an 'I' or 'D' never touches an 'S', an
 *      entry without an '=' run (a read of letters outside the alphabet: mI) is never clipped, sl + sr + the '=' 'X' 'I'
 *      lengths of the kept runs equal the read's length, and the clipped text interval is [start + tl, end - tr).  An entry
 *      gets at most R + 2 runs: the output is allocated at the scripts' n_ops + 2 n_sel and nothing is read back in front of
 *      the write.  n_clipped counts the entries with sl + sr > 0, n_low those with the LOW bit.  An entry with an op other than
 *      = X I D is copied unclipped with score 0, sl = sr = tl = tr = nm = 0 and the LOW bit; with the right handle there are
 *      none.  Every access is bounded by n_sel and n_ops: a foreign handle gives meaningless but harmless results.
 *      tests/clip_naive.py is this contract in executable form.
 *
 *      The clips handle follows the lifecycle of the other chain handles: *inout == NULL allocates, a handle passed in is
 *      reused and its earlier views end; the device arrays (kmx_clips_view_device; cig_off is NULL after a refusal or an error,
 *      the per-entry arrays when n_sel == 0, cigar when n_ops == 0) are complete in stream order when the call returns;
 *      kmx_clips_view copies to page-locked host memory on first use and synchronises, on the stream of the call: 15 bytes per
 *      entry, 8 per entry for cig_off and 4 per run (cig_off always holds at least the one offset 0).  Any output pointer may
 *      be NULL.  The call only reads the scripts and leaves them as they are.
 *
 *      KMX_ERR_INVALID_ARGUMENT before the handle is looked at: a NULL argument, a struct_size that is too small, flags != 0,
 *      match outside 1 .. 255, mismatch, gap_open or gap_extend above 255, clip_penalty above 65535.  After looking: a scripts
 *      handle made with KMX_SCRIPT_M ('=' and 'X' are no longer apart).  After such a refusal or an error the clips handle,
 *      when there is one, holds an empty result.
 *
 *      MD of the clipped entries.  kmx_clips_md (the scripts of kmx_alignments_scripts[_device] or kmx_placements_scripts and
 *      their alignments) and kmx_clips_rescues_md (the scripts of kmx_rescues_scripts and the rescues) apply the rule of
 *      kmx_scripts_md to the runs of the clips, with the text cursor starting at start[sel[e]] + tl[e], the end test against
 *      end[sel[e]] - tr[e], and 'S' treated like 'I'; sel comes from the scripts handle.  An entry with tl + tr > end - start
 *      counts in n_mismatched.  The refusals are those of kmx_scripts_md / kmx_rescues_md; in addition clips whose n_sel
 *      differs from the scripts', or that live on another device, are refused after looking.  The secondaries need no MD here:
 *      XA carries only CIGAR and NM.
 *
 *      Left out: TLEN from the clipped ends, a clip-aware MAPQ and a clip-aware choice between loci (supplementary lines from the
 *      clipped-off part of a read: kmx_clips_supplementaries, below).
 *      Untested: an index with more than one replica, and the different-devices refusals.  kmx_stats_get is not extended (see
 *      kmx_loci_align). */
#define KMX_SOFT_CLIP 1
#define KMX_CLIP_LOW 1u   /* cflags: the best value was below min_score (or the entry has a foreign op): left whole */
typedef struct kmx_clip_options {
    uint32_t struct_size;   /* = sizeof(kmx_clip_options): 32 */
    uint32_t match;         /* a, 1 .. 255 */
    uint32_t mismatch;      /* b, 0 .. 255 */
    uint32_t gap_open;      /* o, 0 .. 255 */
    uint32_t gap_extend;    /* x, 0 .. 255: a gap run of len letters costs o + len x */
    uint32_t clip_penalty;  /* p, 0 .. 65535, charged once per clipped end */
    int32_t min_score;
    uint32_t flags;         /* 0 */
} kmx_clip_options;
typedef struct kmx_clips kmx_clips;
kmx_status kmx_scripts_clip(const kmx_scripts* scripts, const kmx_clip_options* options, void* stream, kmx_clips** inout);
kmx_status kmx_clips_counts(const kmx_clips* c, uint64_t* n_sel, uint64_t* n_ops, uint64_t* n_clipped, uint64_t* n_low);
kmx_status kmx_clips_view(kmx_clips* c, const int32_t** score /* n_sel */, const uint16_t** sl, const uint16_t** sr, const uint16_t** tl,
                          const uint16_t** tr, const uint16_t** nm, const uint8_t** cflags, const uint64_t** cig_off /* n_sel + 1 */,
                          const uint32_t** cigar /* n_ops */);
kmx_status kmx_clips_view_device(const kmx_clips* c, const int32_t** d_score, const uint16_t** d_sl, const uint16_t** d_sr,
                                 const uint16_t** d_tl, const uint16_t** d_tr, const uint16_t** d_nm, const uint8_t** d_cflags,
                                 const uint64_t** d_cig_off, const uint32_t** d_cigar);
kmx_status kmx_clips_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_clips* clips, const kmx_alignments* alignments,
                        const uint8_t* letters, const kmx_md_options* options, void* stream, kmx_md** inout);
kmx_status kmx_clips_rescues_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_clips* clips, const kmx_rescues* rescues,
                                const uint8_t* letters, const kmx_md_options* options, void* stream, kmx_md** inout);
void kmx_clips_free(kmx_clips* c);

/* ---- Realignment: every script aligned again, locally and with affine gaps (an extension, no reference interface; a caller
 *      detects the capability by the macro KMX_REALIGN, KMX_VERSION is unchanged).  Every script of the chain comes from one
 *      unit-cost, end-to-end alignment, and kmx_scripts_clip only trims it: at unit cost a deletion of twelve letters costs what
 *      twelve scattered edits cost, and the canonical walk prefers diagonals, so a long gap comes out in pieces
 *      ('63=1D1=3D2=3D1=3D2=1D1=1D80=' where the read is '70=12D80='), and AS:i is the score of that path.
 *      kmx_scripts_realign aligns every entry of a scripts handle again: a LOCAL, AFFINE-GAP alignment (Gotoh) of the read and
 *      text[start, end), confined to the rectangle and to the band |j - i| <= dist of the script, and fills an ordinary clips
 *      handle.  kmx_clips_md, kmx_clips_supplementaries and the views serve that handle as they serve one of
 *      kmx_scripts_clip; the text interval of entry e still is [start + tl, end - tr).
 *
 *      Input.  The scripts of kmx_alignments_scripts[_device] (KMX_SCRIPT_ALL or not) or of kmx_placements_scripts, the
 *      alignments handle their sel indexes, the index, and the reads that were aligned (for the scripts of the placements: the
 *      doubled batch).  Entry e of the clips is entry e of the scripts.  The host form takes host arrays and runs on the
 *      stream that filled the scripts; the device form takes device arrays and the caller's stream, that stream or one
 *      ordered behind it.
 *
 *      The contract of entry e, with l = sel[e], r = the read with read_sel_off[r] <= e < read_sel_off[r + 1], q = its m
 *      letters, t = text[start[l], end[l]) of L letters, d = dist[l], and the options a = match, b = mismatch, o = gap_open,
 *      x = gap_extend, p = clip_penalty, everything in int64; a gap of len letters costs o + len x, as in kmx_scripts_clip; a
 *      read letter >= sigma equals nothing:
 *        cell (i, j) exists for 0 <= i <= m, 0 <= j <= L, |j - i| <= d; every other cell is -inf in every state;
 *        Z(i) = 0 if i == 0, else -p (a path may begin at any cell, a left clip pays p);
 *        s(i, j) = a if q[i-1] == t[j-1] and q[i-1] < sigma, else -b;
 *        E(i, j) = max(E(i, j-1) - x, H(i, j-1) - o - x)            ends with 'D' (a text letter)
 *        F(i, j) = max(F(i-1, j) - x, H(i-1, j) - o - x)            ends with 'I' (a read letter)
 *        H(i, j) = max(Z(i), H(i-1, j-1) + s(i, j), E(i, j), F(i, j))
 *        V(i, j) = H(i, j) - p [i < m];
 *        the END CELL (i1, j1) has the greatest V; among equals the least i, then the least j;
 *        the WALK starts at (i1, j1) in state H.  State H at (i, j), the first that applies: 1. H == Z(i): stop, (i0, j0) =
 *        (i, j); 2. i, j > 0 and H == H(i-1, j-1) + s: '=' or 'X', to (i-1, j-1) in state H; 3. H == E(i, j): state E;
 *        4. state F.  State E: 'D'; the next state is H if E(i, j) == H(i, j-1) - o - x, else E; to (i, j-1).  State F: the
 *        same with 'I', F, H(i-1, j) and (i-1, j).
 *      The entry is REALIGNED when the path is not empty and V(i1, j1) >= min_score: score[e] = V, sl = i0, sr = m - i1,
 *      tl = j0, tr = L - j1, nm = the 'X' + 'I' + 'D' ops, the runs sl 'S' (only if sl > 0), the ops in forward order as BAM
 *      runs, sr 'S' (only if sr > 0), cflags[e] = KMX_CLIP_REALIGNED.  EVERY OTHER ENTRY is what kmx_scripts_clip makes of a
 *      LOW entry: the script's own runs, score = W[R], sl = sr = tl = tr = 0, nm = the 'X' + 'I' + 'D' lengths of the script,
 *      cflags[e] = KMX_CLIP_LOW.  An entry with runs whose handles do not belong together is such an entry, and neither its read
 *      nor its text is looked at: no such r, a read range that is not one (roff[r] <= roff[r + 1] <= the letters that may be
 *      read), m > KMX_ALIGN_MAX_READ, sel[e] >= n_loci, not start[l] <= end[l] <= n, dist[l] > KMX_ALIGN_MAX_EDITS, or
 *      |m - L| > dist[l].  An entry whose script is empty (mismatched) is not looked at: zeros, no runs, KMX_CLIP_LOW.
 *      n_clipped counts the entries with sl + sr > 0, n_low those with the LOW bit.  So: a clipped side borders an '=' op, the
 *      first and the last kept op never are 'D', the '=' 'X' 'I' lengths sum to i1 - i0 and the '=' 'X' 'D' lengths to
 *      j1 - j0, and with min_score >= 0 score[e] is at least the score[e] of kmx_scripts_clip at the same options: the
 *      trimmed part of the script is one of the paths, and it lies inside the band.  tests/realign_naive.py is this contract
 *      in executable form, cell by cell.
 *
 *      scratch_bytes caps the arena of the traceback codes (0: 256 MiB; an entry takes 32 m bytes per 64 diagonals); the
 *      entries go through it in chunks and the result never depends on it.  Besides the arena the call holds a run
 *      reservation of 4 (m + L + 2) bytes per entry, the bound of a path's runs, for the whole batch.  Every access is bounded
 *      by n_sel, n_loci, roff, m <= KMX_ALIGN_MAX_READ and L <= m + dist: wrong reads or a foreign alignments handle give
 *      meaningless but harmless results.  The call only reads its inputs.
 *
 *      Lifecycle, views and streams are those of the clips handle (above), the roff checks of the host form those of
 *      kmx_alignments_scripts.  A handle may go through kmx_scripts_clip and kmx_scripts_realign in any order.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: a NULL argument, a struct_size that is too small, flags != 0,
 *      match outside 1 .. 255, mismatch, gap_open or gap_extend above 255, clip_penalty above 65535.  After looking: scripts
 *      made with KMX_SCRIPT_M, an nr that differs from the scripts', scripts with more entries than the alignments' n_loci,
 *      handles on different devices, a device without a replica of the index, the host form's roff; KMX_ERR_HIP for an index
 *      broken by kmx_index_extend_query_size_range.  After such a refusal or an error the clips handle, when there is one,
 *      holds an empty result.
 *
 *      Left out: text outside [start, end) and any widening of the band (a better alignment that leaves either is not
 *      found); the scripts of kmx_rescues_scripts and kmx_secondaries_scripts (their sel indexes job arrays, not
 *      alignments); an alignment of the clipped-off letters alone (the tandem duplication of the supplementary alignments,
 *      below); a choice between loci by score and a score-aware MAPQ; kmx_stats_get is not extended (see kmx_loci_align).
 *      Untested: an index with more than one replica, the different-devices refusals, and any batch above the sizes of the
 *      chain's tests (8192 internal reads): no rate at a user's size is claimed. */
#define KMX_REALIGN 1
#define KMX_CLIP_REALIGNED 2u   /* cflags: the entry holds the local affine-gap alignment of kmx_scripts_realign */
typedef struct kmx_realign_options {
    uint32_t struct_size;   /* = sizeof(kmx_realign_options): 40 */
    uint32_t match;         /* a, 1 .. 255 */
    uint32_t mismatch;      /* b, 0 .. 255 */
    uint32_t gap_open;      /* o, 0 .. 255 */
    uint32_t gap_extend;    /* x, 0 .. 255: a gap of len letters costs o + len x */
    uint32_t clip_penalty;  /* p, 0 .. 65535, charged once per clipped end */
    int32_t min_score;
    uint32_t flags;         /* 0 */
    uint64_t scratch_bytes; /* cap on the traceback arena, 0 = 256 MiB; the result never depends on it */
} kmx_realign_options;
kmx_status kmx_scripts_realign(const kmx_index* index, const kmx_alignments* alignments, const kmx_scripts* scripts, const uint8_t* ranks,
                               const uint64_t* roff, uint64_t nr, const kmx_realign_options* options, kmx_clips** inout);
kmx_status kmx_scripts_realign_device(const kmx_index* index, const kmx_alignments* alignments, const kmx_scripts* scripts,
                                      const void* d_ranks, const void* d_roff, uint64_t nr, const kmx_realign_options* options, void* stream,
                                      kmx_clips** inout);

/* ---- Supplementary alignments: the parts of a split read (an extension, no reference interface; a caller detects the
 *      capability by the macro KMX_MAP_SUPPLEMENTARY, KMX_VERSION is unchanged).  Soft clipping marks the part of a read that
 *      does not belong to its placement as 'S'.  A chimeric or split read (across a structural-variant breakpoint, a fusion, a
 *      tandem duplication) is one whose parts belong to different places: the vote gives a locus to each part, kmx_loci_align
 *      aligns the whole read at each, and kmx_scripts_clip trims each script to the part that fits there.  This call picks, on
 *      the device, the clipped entries that cover read letters the primary does not cover: what SAM writes as supplementary
 *      records (FLAG 0x800) and links with SA:Z:.
 *
 *      THE PARTS ARE THE BEST-SCORING PARTS OF THE EDIT-OPTIMAL SCRIPTS, NOT SMITH-WATERMAN REALIGNMENTS: the limit of
 *      kmx_scripts_clip holds here too.  No cell of a dynamic programme is computed again; a part that the unit-cost script of
 *      the whole read at its locus does not contain is not found.
 *
 *      Input.  `reads`, `loci` and `alignments` are those of a doubled batch (nr2 internal reads, nr = nr2 / 2 public ones);
 *      `placements` is the handle of kmx_alignments_fold_strands or of kmx_alignments_fold_pairs, before or after
 *      kmx_pairs_rescue: its locus / strand are read.  `scripts` is kmx_alignments_scripts_device over the doubled reads WITH
 *      KMX_SCRIPT_ALL and without KMX_SCRIPT_M: sel ascends over every aligned locus, read_sel_off[nr2 + 1] runs over the
 *      internal reads.  `clips` is kmx_scripts_clip of those scripts.  `stream` NULL means the stream that filled the clips.  A
 *      caller who passes another stream orders it behind the streams that filled the six handles (a rescue rewrites the
 *      placements on the stream of the chain), and orders the stream of every later call that reads the supplementaries
 *      behind it: the last kernel of this call is left in flight on `stream`, as with the other stream-taking calls of the
 *      chain.  N = max_supplementary.  The call only reads the six handles.
 *
 *      The contract, in int64.  For public read i: m = min(roff2[2i + 1] - roff2[2i], 65535) (the aligner takes no read above
 *      KMX_ALIGN_MAX_READ letters, so a longer read has no entry); ea = read_sel_off[2i], eb = read_sel_off[2i + 1],
 *      ec = read_sel_off[2i + 2], each clamped into [0, n_sel] and made ascending.  Its entries are E = [ea, ec); entry e has
 *      strand s(e) = 0 if e < eb, else 1, and the locus l = sel[e].
 *        The READ INTERVAL of e on the original read is [q0, q1) = [sl[e], m - sr[e]) on strand 0 and [sr[e], m - sl[e]) on
 *        strand 1 (a reverse entry's clip is in the coordinates of the reverse complement).
 *        The TEXT INTERVAL of e is [t0, t1) = [start[l] + tl[e], end[l] - tr[e]).
 *        e HAS RUNS when the clips' cig_off[e + 1] > cig_off[e].
 *        The PRIMARY is the least p in E with sel[p] == locus[i] of the placements.  Read i has no entries and more[i] = 0
 *        when it is unplaced (strand[i] == 255), when it is rescued (locus[i] == 0xFFFFFFFF: the rescue's scripts are a
 *        different handle; left out), when there is no such p, or when p has no runs.
 *        An entry c != p is a CANDIDATE when it has runs, its KMX_CLIP_LOW bit is clear, sel[c] < n_loci,
 *        score[c] >= min_score and q1 - q0 >= min_len.
 *        ov(a, b) = max(0, min(q1_a, q1_b) - max(q0_a, q0_b)).
 *      The greedy selection.  T = {p}.  Repeat: among the candidates not yet taken with ov(c, t) <= max_overlap for EVERY t in
 *      T, find the one with the greatest score, among equals the least e; if there is none, stop with more[i] = 0; if N have
 *      been taken already, stop with more[i] = 1; otherwise take it into T.  TEXT POSITIONS PLAY NO PART IN ADMISSION: a part
 *      may lie on the primary's own text interval, which is what a tandem duplication looks like.  Two loci that describe one
 *      place cover the same read letters, so the read-overlap rule, applied to every member of T, keeps the shadow of the
 *      primary and of every taken part out, as the ELSEWHERE rule does for the secondaries.
 *      The runner-up.  second_score[x] of a taken entry x is the greatest score[c] over the candidates c != x with
 *      ov(c, x) > max_overlap that lie ELSEWHERE from x on the clipped text intervals (s(c) != s(x), or
 *      max(t0_c, t0_x) >= min(t1_c, t1_x): the fold's rule); 0 when there is none (a candidate's score is at least
 *      min_score >= 1, so 0 is unambiguous).
 *
 *      Output.  The taken entries of read i in ASCENDING e.  sup_off[nr + 1] (u64) counts them per PUBLIC read.  Per entry x:
 *      ent[x] (u32, the index into the entries of `scripts` and `clips`: CIGAR, NM and, through kmx_clips_md, MD of the part
 *      are those of that entry, no further kernel is needed), locus[x] (u32), strand[x] (u8), q0[x], q1[x] (u16), t0[x],
 *      t1[x] (u32, the low 32 bits), score[x], second_score[x] (i32), nm[x] (u16) and, when the alignments carry a contig
 *      table, ctg[x] (u32) = the alignments' ctg[locus[x]] (the view is NULL otherwise).  Per public read: more[nr] (u8).
 *      Counters: n_sup = sup_off[nr], n_split = the reads with at least one entry, n_truncated = the reads with more == 1.
 *      Every index is bounded by n_loci, n_sel, nr and the read's own range: foreign or mismatched handles give meaningless but
 *      harmless results (scripts made without KMX_SCRIPT_ALL hold one entry per read, so there are no candidates).
 *      tests/supp_naive.py is this contract in executable form.
 *
 *      The supplementaries handle follows the lifecycle of the other chain handles: *inout == NULL allocates, a handle passed
 *      in is reused and its earlier views end; the device arrays (kmx_supplementaries_view_device; sup_off is NULL after a
 *      refusal or an error, the entry arrays when n_sup == 0, more when nr == 0) are complete in stream order when the call
 *      returns; kmx_supplementaries_view copies to page-locked host memory on first use and synchronises, on the stream of the
 *      call: 31 bytes per entry (35 with ctg), 9 per public read (sup_off always holds at least the one offset 0).  Any output
 *      pointer may be NULL.
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: a NULL argument, a struct_size that is too small, flags != 0,
 *      max_supplementary == 0 or > KMX_SUPPLEMENTARY_MAX, min_len == 0 or > 65535, min_score < 1.  After looking (the
 *      supplementaries handle, when there is one, then holds an empty result): nr2 odd, placements whose 2 nr differs from the
 *      reads' nr2, loci, alignments or scripts whose nr differs from it, loci and alignments that disagree in n_loci, clips
 *      whose n_sel differs from the scripts', scripts made with KMX_SCRIPT_M, handles on different devices;
 *      KMX_ERR_TOO_LARGE when nr * N >= 2^32.
 *
 *      Left out: parts of rescued reads, hard clips, pair-aware parts, a realignment of the part, and scripts only for the
 *      reads whose primary is clipped (KMX_SCRIPT_ALL over every aligned locus is the cost of this call's input).  No call
 *      here writes the SAM lines.  Untested: an index with more than one replica, and the different-devices refusals.
 *      kmx_stats_get is not extended (see kmx_loci_align). */
#define KMX_MAP_SUPPLEMENTARY 1
#define KMX_SUPPLEMENTARY_MAX 8
typedef struct kmx_supplementary_options {
    uint32_t struct_size;        /* = sizeof(kmx_supplementary_options): 24 */
    uint32_t max_supplementary;  /* N, in 1 .. KMX_SUPPLEMENTARY_MAX */
    uint32_t min_len;            /* the read letters a part must keep, 1 .. 65535 */
    uint32_t max_overlap;        /* the read letters a part may share with each part taken before it */
    int32_t min_score;           /* >= 1: the clip score a part needs */
    uint32_t flags;              /* 0 */
} kmx_supplementary_options;
typedef struct kmx_supplementaries kmx_supplementaries;
kmx_status kmx_clips_supplementaries(const kmx_strand_reads* reads, const kmx_loci* loci, const kmx_alignments* alignments,
                                     const kmx_placements* placements, const kmx_scripts* scripts, const kmx_clips* clips,
                                     const kmx_supplementary_options* options, void* stream, kmx_supplementaries** inout);
kmx_status kmx_supplementaries_counts(const kmx_supplementaries* s, uint64_t* nr, uint64_t* n_sup, uint64_t* n_split,
                                      uint64_t* n_truncated);
kmx_status kmx_supplementaries_view(kmx_supplementaries* s, const uint64_t** sup_off /* nr + 1 */, const uint32_t** ent /* n_sup */,
                                    const uint32_t** locus, const uint8_t** strand, const uint16_t** q0, const uint16_t** q1,
                                    const uint32_t** t0, const uint32_t** t1, const int32_t** score, const int32_t** second_score,
                                    const uint16_t** nm, const uint32_t** ctg /* or NULL */, const uint8_t** more /* nr */);
kmx_status kmx_supplementaries_view_device(const kmx_supplementaries* s, const uint64_t** d_sup_off, const uint32_t** d_ent,
                                           const uint32_t** d_locus, const uint8_t** d_strand, const uint16_t** d_q0,
                                           const uint16_t** d_q1, const uint32_t** d_t0, const uint32_t** d_t1, const int32_t** d_score,
                                           const int32_t** d_second_score, const uint16_t** d_nm, const uint32_t** d_ctg,
                                           const uint8_t** d_more);
void kmx_supplementaries_free(kmx_supplementaries* s);

/* ---- Pileup: the chain's alignments counted per text position, and the candidate sites (an extension, no reference
 *      interface; a caller detects the capability by the macro KMX_PILEUP, KMX_VERSION is unchanged).  Every other stage
 *      turns per-locus data into a per-read answer; kmx_clips_pileup_device / kmx_clips_rescues_pileup turn the per-read
 *      answers (the runs of a scripts or clips handle, the clipped text interval, KMX_CLIP_LOW, the score, a MAPQ array)
 *      into a per-text-position answer on the device, and kmx_pileup_sites into the few positions worth looking at.
 *
 *      The pileup handle holds, for a text region [lo, hi) of len = hi - lo positions, C = sigma + 3 planes of uint32
 *      counters, CHANNEL-MAJOR: counts[c len + (pos - lo)].  Channel c < sigma: a read letter of rank c aligned ('=' or 'X')
 *      to the position; c = sigma (OTHER): an aligned read letter >= sigma; c = sigma + 1 (DEL): the position lies inside a
 *      'D' run; c = sigma + 2 (INS): an 'I' run lies between the position and the next, counted once per run at the text
 *      letter in front of it (the VCF anchor).  The layout is ABI.  Counters wrap modulo 2^32; nothing guards that.
 *
 *      Input.  kmx_clips_pileup_device serves the scripts of kmx_alignments_scripts[_device] and kmx_placements_scripts: sel
 *      indexes the alignments' start / end, and d_ranks / d_roff / nr are the reads that were aligned, on the device (for
 *      the scripts of the placements: the doubled batch).  kmx_clips_rescues_pileup serves the scripts of
 *      kmx_rescues_scripts: sel indexes the rescue's jobs, and the reads are the doubled batch of `reads`.  `clips` is the
 *      clips handle of those scripts (kmx_scripts_clip or kmx_scripts_realign), or NULL: the scripts' own runs then, with
 *      tl = tr = 0, no score and no cflags.  d_mapq is a raw device array (kmx_mapq_view_device) that is read at r >> 1 for
 *      internal read r, so it means something only over a doubled batch; NULL: no MAPQ filter.  `stream` NULL means the
 *      stream that filled the scripts.  The calls only read their inputs.
 *
 *      The contract of entry e, in int64 (tests/pileup_naive.py is this text in executable form).  The runs are the
 *      clips' when given, else the scripts'; l = sel[e]; r = the internal read with read_sel_off[r] <= e <
 *      read_sel_off[r + 1], m its length, q its letters; s = start[l], t = end[l]; tl, tr, score, cflags are the clips', or 0.
 *      In this order:
 *        1. No runs: nothing happens, no counter moves.
 *        2. FILTERED (n_filtered) when KMX_PILEUP_SKIP_LOW is set, clips are given and cflags & KMX_CLIP_LOW; or clips are
 *           given and score < min_score; or d_mapq is given, there is such an r, and d_mapq[r >> 1] < min_mapq.
 *        3. MISMATCHED (n_mismatched, nothing added) when l >= the bound of start / end; there is no such r (or its roff
 *           range is not one); not s <= t <= n; tl + tr > t - s; an op other than = X I D S; an S run that is neither the
 *           first nor the last run; the = X D lengths differ from t - s - tl - tr; the = X I S lengths differ from m.  One
 *           pass over the runs decides this in front of any add.
 *        4. Otherwise ADDED (n_added).  t0 = s + tl, t1 = t - tr, cursors i = 0, j = t0.  'S': i += len.  '=' / 'X': for
 *           each letter x, add(q[i + x] < sigma ? q[i + x] : sigma, j + x); both cursors advance.  'D': add(DEL, j + x) for
 *           each x; j advances.  'I': if t0 < j < t1, add(INS, j - 1) once; i advances (a terminal 'I' run is an overhang,
 *           which SAM would clip: not counted).  add(c, pos) does something only for lo <= pos < hi: the counter goes up
 *           by one, and so does n_cells.
 *      Internal read 2i + 1 of a doubled batch already is the reverse complement: its letters are in text orientation,
 *      nothing is strand-specific.  Every access is bounded by n_sel, n_ops, the bound, nr, the read's own range and the
 *      region: foreign handles give meaningless but harmless counts.
 *
 *      Lifecycle.  *inout == NULL allocates the handle and zeroes the planes of the call's region (hi == 0: the text length
 *      n).  A handle passed in without KMX_PILEUP_ADD is re-made for the call's region and zeroed; with KMX_PILEUP_ADD the
 *      call adds to what is there (to zeroed planes when the handle holds nothing), and is refused, the handle untouched,
 *      when lo, hi or sigma differ from the handle's.  The counters of kmx_pileup_counts are cumulative since the planes
 *      were last zeroed.  THE CALL DOES NOT SYNCHRONISE: it leaves its kernels in flight on `stream` and reads nothing
 *      back.  kmx_pileup_counts and kmx_pileup_view synchronise on the stream of the
 *      last call; kmx_pileup_view fills page-locked host memory (4 C len bytes), kmx_pileup_view_device returns the device
 *      pointer (NULL for a handle that holds nothing).  Streams between calls, and the scratch of the handle that two calls
 *      share, are the caller's to order, as elsewhere in the chain.
 *
 *      mode and tile are knobs like scratch_bytes: THE RESULT NEVER DEPENDS ON THEM.  KMX_PILEUP_ATOMIC: a wave per entry,
 *      the lanes on consecutive positions of a plane, global atomic adds.  KMX_PILEUP_TILED (the region in tiles of `tile`
 *      positions, a workgroup per tile that counts in LDS and adds its planes with plain loads and stores) was built and
 *      measured, lost to the atomic path at every shape that was probed, and is not in the library:
 *      KMX_PILEUP_TILED AND KMX_PILEUP_AUTO RUN THE ATOMIC PATH, and `tile` is checked and otherwise ignored.  Both fields
 *      stay so that a path for batches the probe could not reach can come back without a change of the ABI.
 *
 *      kmx_pileup_sites: for every pos in [lo, hi), ref = text[pos]; depth = the sum of the channels 0 .. sigma + 1 in
 *      uint64; the position is skipped when depth < max(min_depth, 1), else it counts in n_covered.  The candidates, in
 *      ascending channel order, are the letters c < sigma with c != ref, then DEL, then INS (OTHER never is one); a
 *      candidate passes when cnt >= max(min_alt, 1) and cnt frac_den >= frac_num depth, in integers.  One record per
 *      passing (pos, channel), ordered by (pos, channel): pos (u32), ref, alt (u8; alt is a channel), depth, count,
 *      ref_count (u32; depth saturated) and, when the index has a contig table, ctg (u32; the view is NULL otherwise).  A
 *      deletion is reported per deleted position.  The sites handle follows the lifecycle of the other chain handles (the
 *      call synchronises: one read-back sizes the records; `stream` NULL means the stream of the pileup's last call).
 *
 *      KMX_ERR_INVALID_ARGUMENT before any handle is looked at: a NULL argument (clips and d_mapq may be NULL), a
 *      struct_size that is too small, unknown flag bits, mode > 2, a tile that is neither 0 nor a power of two >= 64; for
 *      the sites frac_den == 0 or frac_num > frac_den.  After looking: lo >= hi or hi > n, scripts made with KMX_SCRIPT_M,
 *      clips whose n_sel differs from the scripts', an nr that differs from the scripts', an odd nr with d_mapq, handles on
 *      different devices, a device without a replica of the index, the KMX_PILEUP_ADD mismatch; KMX_ERR_HIP for an index
 *      broken by kmx_index_extend_query_size_range; for the sites a pileup that holds nothing, or whose channels are not
 *      sigma + 3 or whose hi > n.  After such a refusal a pileup handle that was passed in holds nothing, unless
 *      KMX_PILEUP_ADD was set: then it is untouched.  After an error of the device it holds nothing.
 *
 *      Left out: merging deleted positions into one indel record, the inserted letters, base qualities, a VCF writer, the
 *      scripts of kmx_secondaries_scripts.  Untested: an index with more than one replica, the different-devices refusals,
 *      and any batch above the sizes of the chain's tests (8192 internal reads).  kmx_stats_get is not extended. */
#define KMX_PILEUP 1
#define KMX_PILEUP_ADD      1u   /* flags: add to the planes the handle holds */
#define KMX_PILEUP_SKIP_LOW 2u   /* flags: entries whose clips carry KMX_CLIP_LOW are FILTERED */
#define KMX_PILEUP_AUTO   0u
#define KMX_PILEUP_ATOMIC 1u
#define KMX_PILEUP_TILED  2u
typedef struct kmx_pileup_options {
    uint32_t struct_size;   /* = sizeof(kmx_pileup_options): 40 */
    uint32_t flags;         /* KMX_PILEUP_ADD | KMX_PILEUP_SKIP_LOW */
    uint64_t lo, hi;        /* the region; hi == 0: the text length n */
    int32_t min_score;      /* entries whose clips score less are FILTERED */
    uint32_t min_mapq;      /* entries whose read's MAPQ is less are FILTERED (with d_mapq) */
    uint32_t mode;          /* KMX_PILEUP_AUTO, _ATOMIC or _TILED; the result never depends on it (all three run the atomic path) */
    uint32_t tile;          /* 0, or a power of two >= 64; checked, otherwise ignored (see above) */
} kmx_pileup_options;
typedef struct kmx_sites_options {
    uint32_t struct_size;   /* = sizeof(kmx_sites_options): 20 */
    uint32_t min_depth;
    uint32_t min_alt;
    uint32_t frac_num;      /* a candidate needs cnt frac_den >= frac_num depth */
    uint32_t frac_den;
} kmx_sites_options;
typedef struct kmx_pileup kmx_pileup;
typedef struct kmx_sites kmx_sites;
kmx_status kmx_clips_pileup_device(const kmx_index* index, const kmx_alignments* alignments, const kmx_scripts* scripts,
                                   const kmx_clips* clips /* or NULL */, const void* d_ranks, const void* d_roff, uint64_t nr,
                                   const uint8_t* d_mapq /* nr / 2, or NULL */, const kmx_pileup_options* options, void* stream,
                                   kmx_pileup** inout);
kmx_status kmx_clips_rescues_pileup(const kmx_index* index, const kmx_strand_reads* reads, const kmx_rescues* rescues,
                                    const kmx_scripts* scripts, const kmx_clips* clips /* or NULL */, const uint8_t* d_mapq /* or NULL */,
                                    const kmx_pileup_options* options, void* stream, kmx_pileup** inout);
kmx_status kmx_pileup_counts(kmx_pileup* p, uint64_t* lo, uint64_t* hi, uint32_t* n_channels, uint64_t* n_added, uint64_t* n_filtered,
                             uint64_t* n_mismatched, uint64_t* n_cells);
kmx_status kmx_pileup_view(kmx_pileup* p, const uint32_t** counts /* n_channels * (hi - lo) */);
kmx_status kmx_pileup_view_device(const kmx_pileup* p, const uint32_t** d_counts);
void kmx_pileup_free(kmx_pileup* p);
kmx_status kmx_pileup_sites(const kmx_index* index, const kmx_pileup* pileup, const kmx_sites_options* options, void* stream,
                            kmx_sites** inout);
kmx_status kmx_sites_counts(const kmx_sites* s, uint64_t* n_sites, uint64_t* n_covered);
kmx_status kmx_sites_view(kmx_sites* s, const uint32_t** pos /* n_sites */, const uint8_t** ref, const uint8_t** alt, const uint32_t** depth,
                          const uint32_t** count, const uint32_t** ref_count, const uint32_t** ctg /* or NULL */);
kmx_status kmx_sites_view_device(const kmx_sites* s, const uint32_t** d_pos, const uint8_t** d_ref, const uint8_t** d_alt,
                                 const uint32_t** d_depth, const uint32_t** d_count, const uint32_t** d_ref_count, const uint32_t** d_ctg);
void kmx_sites_free(kmx_sites* s);

/* The text, reconstructed on the device from the index (an extension, no reference interface): every offset 0 .. n-k of one
 * element's contiguous copy of the buckets names the first letter of its k-mer, the index's tail gives the last k-1 letters.
 * Works on built, loaded and replicated indexes (this replica).  The first call derives a copy packed at 2, 4 or 8 bits per
 * letter (sigma <= 4, <= 16, else), which stays on the device until kmx_index_free (kmx_search_approx reads it; it is not part
 * of kmx_index_memory).  out_ranks may be NULL: only derive the packed copy and report its size in *packed_bytes (may be
 * NULL); otherwise n must be the index's text length and out_ranks receives the n letters as ranks. */
kmx_status kmx_index_text(const kmx_index* index, uint8_t* out_ranks, uint64_t n, uint64_t* packed_bytes);

/* Timing of the kernels launched for this index since the last reset (HIP events on
 * the stream each kernel ran on).  Enabled by kmx_stats_enable(index, 1). */
kmx_status kmx_stats_enable(kmx_index* index, int enable);
kmx_status kmx_stats_get(kmx_index* index, kmx_kernel_stat* stats /* KMX_N_KERNELS */, uint32_t* n);
kmx_status kmx_stats_reset(kmx_index* index);

/* Debug aid: 16 words of range-violation records written by -DKMX_CHECKED builds (word 0 = count;
 * always 0 in a normal build). */
kmx_status kmx_debug_words(const kmx_index* index, uint64_t* words16);

const char* kmx_last_error(void);
const char* kmx_status_string(kmx_status s);
uint32_t kmx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KMX_H */
