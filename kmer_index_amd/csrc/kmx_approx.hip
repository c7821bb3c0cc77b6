// Approximate search (kmx_search_approx, include/kmx.h): every window of the text within Hamming distance e <= 3 of a query.
//
// Pigeonhole seeding: a query of m letters is cut into e + 1 pieces; a window with at most e substitutions matches one
// of them exactly.  The pieces tile the query and the queries tile the letters of the batch, so the piece batch is the
// same letters with a finer offset array (k_approx_prep); it goes through the exact batch search unchanged
// (kmx_search_batch_device: whatever the piece length, exact, stitched, sub-k or multi-k).  Each piece hit h of piece j
// names the window p = h - off_j; k_approx_verify compares it with the query on a packed copy of the text (2 / 4 / 8 bits
// per letter, derived from the index: k_text_scatter + k_text_pack) and keeps it when it has at most e mismatches AND no
// piece before j matches the window exactly (the first-exact-piece rule: every window is reported by exactly one piece,
// so nothing needs deduplicating).  The survivors of each (query, piece) list stay ascending; k_approx_compact packs them
// in candidate order and k_approx_merge places each at its rank among the survivors of the query's other lists.
// With KMX_APPROX_EDIT (edit distance: insertions and deletions too) the piece search is the same and a second path follows
// it: see "edit distance" below.  kmx_search_approx_strands runs every query and its reverse complement through the same
// pipeline as one batch of twice the queries: see "both strands" below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "kmx_approx.h"
#include "kmx_handle.h"
#include "kmx_kernels.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kVerifyCpt = 4;                       // candidates per thread of k_approx_verify / k_approx_compact
constexpr uint64_t kVerifySpan = uint64_t(kBlock) * kVerifyCpt;
constexpr uint64_t kMaxPieces = uint64_t(1) << 25;       // pieces per exact search (the exact host path's pass size)
constexpr uint64_t kDefaultBudget = uint64_t(1) << 29;   // piece hits (candidates) per chunk

inline uint32_t bits_per_letter(uint32_t sigma) { return sigma <= 4 ? 2u : sigma <= 16 ? 4u : 8u; }

using kmx::Buf;
using kmx::DeviceGuard;
using kmx::PinnedArr;
using kmx::grid_for;

} // namespace

struct kmx_approx_result {
    uint64_t nq = 0, n_hits = 0, n_candidates = 0;
    uint32_t n_chunks = 0;
    bool edit = false;                                   // KMX_APPROX_EDIT: mismatches holds distances, lengths is filled
    bool strands = false;                                // kmx_search_approx_strands: strand is filled
    bool opts = false;                                   // kmx_search_approx_opts: kmx_approx_found works
    bool reported = false;                               // ... with a reporting option: found is filled by the device stage
    PinnedArr hit_off, positions, mismatches, status, lengths, strand, found;
    std::vector<uint64_t> found_lazy;                    // opts && !reported: the list lengths, made by the first kmx_approx_found
};

// ------------------------------------------------------------------------------------------------------------------------
// kernels

// One thread per entry of the element's contiguous copy: its group (binary search of offs) names the key, whose first letter
// is the text letter at the entry's position.  Every offset 0 .. n - k is written exactly once.
__global__ __launch_bounds__(kBlock) void k_text_scatter(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ offs,
                                                         const uint64_t* __restrict__ ukeys, uint64_t n_groups, uint64_t npos,
                                                         uint64_t div, uint64_t n, uint8_t* __restrict__ t8)
{
    for (uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x; t < npos; t += uint64_t(gridDim.x) * kBlock) {
        uint64_t lo = 0, hi = n_groups;               // offs[lo] <= t < offs[hi] (offs[n_groups] == npos)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (offs[mid] <= t) lo = mid; else hi = mid;
        }
        const uint64_t key = ukeys ? ukeys[lo] : lo;
        const uint32_t p = pos[t];
        if (p < n) t8[p] = uint8_t(key / div);
    }
}

// word i <- letters [i * L, (i + 1) * L) at w bits each from bit 0; words past the text are zero
__global__ __launch_bounds__(kBlock) void k_text_pack(const uint8_t* __restrict__ t8, uint64_t n, uint32_t w, uint64_t n_words,
                                                      uint64_t* __restrict__ words)
{
    const uint32_t L = 64 / w;
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n_words; i += uint64_t(gridDim.x) * kBlock) {
        uint64_t v = 0;
        const uint64_t a = i * L;
        for (uint32_t r = 0; r < L && a + r < n; ++r) v |= uint64_t(t8[a + r]) << (r * w);
        words[i] = v;
    }
}

__global__ __launch_bounds__(kBlock) void k_text_unpack(const uint64_t* __restrict__ words, uint64_t n, uint32_t w, uint8_t* __restrict__ out)
{
    const uint32_t L = 64 / w;
    const uint64_t mask = (uint64_t(1) << w) - 1;
    for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock)
        out[i] = uint8_t((words[i / L] >> ((i % L) * w)) & mask);
}

// piece j of a query of m letters: [start(j), start(j + 1)), the first m mod (e + 1) pieces one letter longer
__device__ __forceinline__ uint64_t piece_start(uint64_t m, uint32_t e, uint32_t j)
{
    const uint64_t base = m / (e + 1), rem = m % (e + 1);
    return j * base + min(uint64_t(j), rem);
}

// One thread per query: its status from the query alone, its piece offsets (e + 1 per query, absolute in qr), its letters
// packed at w bits (from word qoff[i] / L + i: queries never share a word).  The letters of a query that cannot be served are
// overwritten with 255 where that is outside the alphabet, so that none of its pieces costs the exact search anything.
__global__ __launch_bounds__(kBlock) void k_approx_prep(uint8_t* __restrict__ qr, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                        uint32_t sigma, uint32_t e, uint32_t range, uint32_t w,
                                                        uint64_t* __restrict__ poff, uint8_t* __restrict__ qstat,
                                                        uint64_t* __restrict__ qwords)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= nq) return;
    const uint64_t a = qoff[i], m = qoff[i + 1] - a;
    const uint32_t L = 64 / w;
    uint8_t st = KMX_Q_OK;
    if (m == 0) st = KMX_Q_EMPTY_QUERY;
    else if (m <= e) st = KMX_Q_TOO_SHORT;
    else if ((m + e) / (e + 1) >= range) st = KMX_Q_TOO_LONG;
    else {
        uint64_t* qw = qwords + a / L + i;
        uint64_t v = 0;
        for (uint64_t r = 0; r < m; ++r) {
            const uint32_t c = qr[a + r];
            if (c >= sigma) st = KMX_Q_BAD_RANK;
            v |= uint64_t(c & ((1u << w) - 1)) << ((r % L) * w);
            if (r % L == L - 1 || r + 1 == m) { qw[r / L] = v; v = 0; }
        }
    }
    qstat[i] = st;
    for (uint32_t j = 0; j <= e; ++j) poff[i * (e + 1) + j] = a + piece_start(m, e, j);
    if (i + 1 == nq) poff[nq * (e + 1)] = qoff[nq];
    if (st != KMX_Q_OK && sigma < 256)
        for (uint64_t r = 0; r < m; ++r) qr[a + r] = 255;
}

// queries [0, nq) of the chunk: candidates in front of each (the piece hit offsets of its first piece)
__global__ __launch_bounds__(kBlock) void k_approx_query_cands(const uint64_t* __restrict__ phit, uint64_t nq, uint32_t e,
                                                               uint64_t* __restrict__ qcand)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i <= nq) qcand[i] = phit[i * (e + 1)];
}

// a served query one of whose pieces the exact search refused (sub-k fan-out) takes that status
__global__ __launch_bounds__(kBlock) void k_approx_status(const uint8_t* __restrict__ pstat, uint64_t nq, uint32_t e,
                                                          uint8_t* __restrict__ qstat)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= nq || qstat[i] != KMX_Q_OK) return;
    for (uint32_t j = 0; j <= e; ++j) {
        const uint8_t s = pstat[i * (e + 1) + j];
        if (s != KMX_Q_OK) { qstat[i] = s; return; }
    }
}

struct VerifyArgs {
    const uint64_t* phit;     // [np + 1] piece hit offsets (the exact search's hit_off over the pieces)
    const uint32_t* pos;      // [n_cand] piece hits
    uint64_t n_cand, np;
    const uint64_t* qoff;     // query offsets of the chunk's letters; query of piece P is q0 + P / (e + 1)
    uint64_t q0;
    const uint8_t* qstat;
    const uint64_t* qwords;
    const uint64_t* text;     // packed text
    uint64_t n;
    uint32_t w, e;
    uint8_t* keep;            // [n_cand]: mismatches of a kept window, 0xFF otherwise
    uint32_t* bcount;         // kept windows per block
};

// last piece P in [lo, hi) with phit[P] <= c
__device__ __forceinline__ uint64_t piece_of(const uint64_t* __restrict__ phit, uint64_t lo, uint64_t hi, uint64_t c)
{
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (phit[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// one bit per letter (its lowest) of the w-bit fields of x that are not zero
__device__ __forceinline__ uint64_t fold(uint64_t x, uint32_t w)
{
    if (w == 2) return (x | (x >> 1)) & 0x5555555555555555ull;
    if (w == 4) { x |= x >> 1; x |= x >> 2; return x & 0x1111111111111111ull; }
    x |= x >> 1; x |= x >> 2; x |= x >> 4;
    return x & 0x0101010101010101ull;
}

// Candidate-parallel: a block takes kVerifySpan consecutive piece hits (whatever lists they belong to), thread t those at
// t, t + 256, ...  Each one is a window of the text read as two-word funnel shifts from the packed copy (L2 / Infinity-Cache
// resident: 25 MB for 10^8 DNA letters), XORed with the packed query; the count stops at e + 1.
__global__ __launch_bounds__(kBlock) void k_approx_verify(VerifyArgs A)
{
    __shared__ uint64_t s_range[2];
    const uint64_t c0 = uint64_t(blockIdx.x) * kVerifySpan;
    const uint64_t c_end = min(c0 + kVerifySpan, A.n_cand);
    if (threadIdx.x == 0) {
        s_range[0] = piece_of(A.phit, 0, A.np, c0);
        s_range[1] = piece_of(A.phit, s_range[0], A.np, c_end - 1) + 1;
    }
    __syncthreads();
    const uint64_t plo = s_range[0], phi = s_range[1];
    const uint32_t e = A.e, w = A.w, L = 64 / w;
    uint32_t kept_here = 0;
    for (uint32_t it = 0; it < kVerifyCpt; ++it) {
        const uint64_t c = c0 + uint64_t(it) * kBlock + threadIdx.x;
        uint8_t out = 0xFF;
        if (c < c_end) {
            const uint64_t P = piece_of(A.phit, plo, phi, c);
            const uint64_t qi = A.q0 + P / (e + 1);
            const uint32_t j = uint32_t(P % (e + 1));
            const uint64_t a = A.qoff[qi], m = A.qoff[qi + 1] - a;
            const uint64_t h = A.pos[c], oj = piece_start(m, e, j);
            if (A.qstat[qi] == KMX_Q_OK && h >= oj && h - oj + m <= A.n) {
                const uint64_t p = h - oj;
                const uint64_t* __restrict__ qw = A.qwords + a / L + qi;
                const uint64_t nw = (m + L - 1) / L;
                const uint64_t bit = p * w;
                const uint64_t* __restrict__ tw = A.text + (bit >> 6);
                const uint32_t sh = uint32_t(bit & 63);
                uint64_t lo = tw[0];
                uint32_t cnt = 0;
                uint32_t mm[KMX_APPROX_MAX_SUBST];
                bool over = false;
                for (uint64_t t = 0; t < nw; ++t) {
                    const uint64_t hi = tw[t + 1];
                    const uint64_t x = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
                    lo = hi;
                    uint64_t f = fold(x ^ qw[t], w);
                    if (t + 1 == nw) {
                        const uint64_t rb = (m - t * L) * w;           // bits of the last word that hold letters
                        if (rb < 64) f &= (uint64_t(1) << rb) - 1;
                    }
                    if (!f) continue;
                    const uint32_t k = uint32_t(__popcll(f));
                    if (cnt + k > e) { over = true; break; }
                    while (f) {
                        mm[cnt++] = uint32_t(t * L + uint32_t(__ffsll((long long)f) - 1) / w);
                        f &= f - 1;
                    }
                }
                if (!over) {
                    // first-exact-piece rule: every piece in front of j has a mismatch
                    bool first = true;
                    for (uint32_t jj = 0; jj < j; ++jj) {
                        const uint64_t s = piece_start(m, e, jj), s2 = piece_start(m, e, jj + 1);
                        bool hit = false;
                        for (uint32_t r = 0; r < cnt; ++r) hit |= mm[r] >= s && mm[r] < s2;
                        first &= hit;
                    }
                    if (first) out = uint8_t(cnt);
                }
            }
            A.keep[c] = out;
        }
        kept_here += __syncthreads_count(out != 0xFF);
    }
    if (threadIdx.x == 0) A.bcount[blockIdx.x] = kept_here;
}

// The kept windows in candidate order (= by piece, ascending inside a piece): block b writes from bscan[b].
__global__ __launch_bounds__(kBlock) void k_approx_compact(VerifyArgs A, const uint64_t* __restrict__ bscan,
                                                           uint32_t* __restrict__ s_pos, uint32_t* __restrict__ s_piece,
                                                           uint8_t* __restrict__ s_mm)
{
    __shared__ uint32_t wave_n[kBlock / 64];
    __shared__ uint64_t s_range[2];
    const uint64_t c0 = uint64_t(blockIdx.x) * kVerifySpan;
    const uint64_t c_end = min(c0 + kVerifySpan, A.n_cand);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (A.bcount[blockIdx.x] == 0) return;                      // (block-uniform)
    if (threadIdx.x == 0) {                                     // the pieces this block's candidates belong to
        s_range[0] = piece_of(A.phit, 0, A.np, c0);
        s_range[1] = piece_of(A.phit, s_range[0], A.np, c_end - 1) + 1;
    }
    uint64_t base = bscan[blockIdx.x];
    for (uint32_t it = 0; it < kVerifyCpt; ++it) {
        const uint64_t c = c0 + uint64_t(it) * kBlock + threadIdx.x;
        const uint8_t k = c < c_end ? A.keep[c] : uint8_t(0xFF);
        const bool kept = k != 0xFF;
        const uint64_t ball = __ballot(kept);
        if (lane == 0) wave_n[wv] = uint32_t(__popcll(ball));
        __syncthreads();
        uint64_t at = base;
        uint32_t total = 0;
        for (uint32_t v = 0; v < kBlock / 64; ++v) {
            if (v < wv) at += wave_n[v];
            total += wave_n[v];
        }
        if (kept) {
            at += __popcll(ball & ((uint64_t(1) << lane) - 1));
            const uint64_t P = piece_of(A.phit, s_range[0], s_range[1], c);
            const uint64_t qi = A.q0 + P / (A.e + 1);
            const uint64_t m = A.qoff[qi + 1] - A.qoff[qi];
            s_pos[at] = uint32_t(A.pos[c] - piece_start(m, A.e, uint32_t(P % (A.e + 1))));
            s_piece[at] = uint32_t(P);
            s_mm[at] = k;
        }
        base += total;
        __syncthreads();
    }
}

// first index in [lo, hi) with a[i] >= x
__device__ __forceinline__ uint64_t lower_u32(const uint32_t* __restrict__ a, uint64_t lo, uint64_t hi, uint32_t x)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// hit_off of the chunk's queries: the start of each query's survivors (s_piece is ascending)
__global__ __launch_bounds__(kBlock) void k_approx_hit_off(const uint32_t* __restrict__ s_piece, uint64_t n_s, uint64_t nq, uint32_t e,
                                                           uint64_t* __restrict__ hit_off)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i <= nq) hit_off[i] = i == nq ? n_s : lower_u32(s_piece, 0, n_s, uint32_t(i * (e + 1)));
}

// Survivor s of list P (query i, piece j) goes to: the query's first slot + its rank in its own list + the survivors of the
// query's other lists below it (the lists hold distinct windows: the first-exact-piece rule).
__global__ __launch_bounds__(kBlock) void k_approx_merge(const uint32_t* __restrict__ s_pos, const uint32_t* __restrict__ s_piece,
                                                         const uint8_t* __restrict__ s_mm, uint64_t n_s, uint32_t e,
                                                         uint32_t* __restrict__ out_pos, uint8_t* __restrict__ out_mm)
{
    const uint64_t s = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (s >= n_s) return;
    const uint32_t P = s_piece[s], p = s_pos[s];
    const uint32_t first = P - P % (e + 1);
    const uint64_t own = lower_u32(s_piece, 0, n_s, P);
    uint64_t dest = lower_u32(s_piece, 0, n_s, first) + (s - own);
    for (uint32_t j = 0; j <= e; ++j) {
        if (first + j == P) continue;
        const uint64_t lo = lower_u32(s_piece, 0, n_s, first + j), hi = lower_u32(s_piece, lo, n_s, first + j + 1);
        dest += lower_u32(s_pos, lo, hi, p) - lo;
    }
    out_pos[dest] = p;
    out_mm[dest] = s_mm[s];
}

// ------------------------------------------------------------------------------------------------------------------------
// edit distance (KMX_APPROX_EDIT): the same pieces, a banded dynamic programme per piece hit instead of the XOR
//
// A window within e edits of the query holds one piece exactly, at most e letters off its nominal offset: piece hit h of
// piece j names the diagonal D = h - o_j and the starts p = D - e .. D + e.  k_edit_verify computes d(p) for all of them in
// one pass from the end of the query to its front (F[i][t] = least distance of q[i, m) to a window that starts at t; a path
// of cost <= e from a start within e of D stays on the 4e + 1 diagonals around D), k_edit_emit turns the survivors into
// (query, p) keys, the radix sort of kmx_build_sort.hip orders them, equal neighbours are dropped, and k_edit_lengths runs
// a forward pass of 2e + 1 diagonals from every remaining start for its window length.

constexpr uint32_t kEditInf = 8;                     // any distance > KMX_APPROX_MAX_SUBST; cells saturate here
constexpr uint32_t kEditNone = 7;                    // 3-bit field of EditArgs::keep: the start is no hit

struct EditArgs {
    const uint64_t* phit;     // as VerifyArgs
    const uint32_t* pos;
    uint64_t n_cand, np;
    const uint64_t* qoff;
    uint64_t q0;
    const uint8_t* qstat;
    const uint64_t* qwords;
    const uint64_t* text;
    uint64_t n;
    uint32_t e;
    uint32_t* keep;           // [n_cand]: 3 bits per start D - e .. D + e, its distance or kEditNone
    uint32_t* bcount;         // surviving starts per block
};

// Letters tlo + r (r = 0 .. NL - 1) of the packed text against letter c: bit r * W of f0 (r < 64 / W) or bit (r - 64 / W) * W of
// f1 is set when they differ.  Letters in front of the text or past it come out arbitrary (the callers' cells there are
// invalid); no word outside the allocation is read (tlo is clamped to [0, n], three words from there lie inside the padding).
template <uint32_t W, uint32_t NL>
__device__ __forceinline__ void window_neq(const uint64_t* __restrict__ text, int64_t tlo, uint64_t n, uint32_t c, uint64_t& f0, uint64_t& f1)
{
    constexpr bool two = NL * W > 64;
    const int64_t tb = min(max(tlo, int64_t(0)), int64_t(n));
    const uint64_t bit = uint64_t(tb) * W;
    const uint64_t* __restrict__ tw = text + (bit >> 6);
    const uint32_t sh = uint32_t(bit & 63);
    const uint64_t w0 = tw[0], w1 = tw[1];
    uint64_t x0 = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0, x1 = 0;
    if (two) {
        const uint64_t w2 = tw[2];
        x1 = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
    }
    if (tlo < 0) {                                   // letter 0 of the text belongs at field -tlo
        const uint64_t s = min(uint64_t(-tlo) * W, uint64_t(two ? 127 : 63));
        if (two) {
            if (s >= 64) { x1 = x0 << (s - 64); x0 = 0; }
            else { x1 = (x1 << s) | (x0 >> (64 - s)); x0 <<= s; }
        } else {
            x0 <<= s;
        }
    }
    const uint64_t rep = uint64_t(c) * (W == 2 ? 0x5555555555555555ull : W == 4 ? 0x1111111111111111ull : 0x0101010101010101ull);
    f0 = fold(x0 ^ rep, W);
    f1 = two ? fold(x1 ^ rep, W) : 0;
}

template <uint32_t W>
__device__ __forceinline__ uint32_t neq_at(uint64_t f0, uint64_t f1, uint32_t r)
{
    constexpr uint32_t L = 64 / W;
    return uint32_t((r < L ? f0 >> (r * W) : f1 >> ((r - L) * W)) & 1u);
}

template <uint32_t W>
__device__ __forceinline__ uint32_t query_letter(const uint64_t* __restrict__ qw, uint64_t i)
{
    constexpr uint32_t L = 64 / W;
    return uint32_t(qw[i / L] >> ((i % L) * W)) & ((1u << W) - 1);
}

// Candidate-parallel like k_approx_verify.  Cell r of a row is the diagonal D + r - 2E: row i, text offset t = i + D + r - 2E.
//   F[m][t] = 0,  F[i][t] = min(F[i + 1][t + 1] + (q[i] != text[t]), F[i + 1][t] + 1, F[i][t + 1] + 1),  t <= n, nothing past n
// so a row is updated in place from its last cell to its first; the row of 4E + 1 cells stays in registers (every index is a
// compile-time constant).  A cell with t < 0 holds no meaning and feeds none with t >= 0 (a cell depends on t and t + 1 only).
template <uint32_t E, uint32_t W>
__global__ __launch_bounds__(kBlock) void k_edit_verify(EditArgs A)
{
    constexpr uint32_t NB = 4 * E + 1, L = 64 / W;
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_kept;
    const uint64_t c0 = uint64_t(blockIdx.x) * kVerifySpan;
    const uint64_t c_end = min(c0 + kVerifySpan, A.n_cand);
    if (threadIdx.x == 0) {
        s_range[0] = piece_of(A.phit, 0, A.np, c0);
        s_range[1] = piece_of(A.phit, s_range[0], A.np, c_end - 1) + 1;
        s_kept = 0;
    }
    __syncthreads();
    const uint64_t plo = s_range[0], phi = s_range[1];
    const int64_t n = int64_t(A.n);
    uint32_t kept_here = 0;
    for (uint32_t it = 0; it < kVerifyCpt; ++it) {
        const uint64_t c = c0 + uint64_t(it) * kBlock + threadIdx.x;
        if (c >= c_end) break;
        uint32_t out = 0;
#pragma unroll
        for (uint32_t k = 0; k <= 2 * E; ++k) out |= kEditNone << (3 * k);
        const uint64_t P = piece_of(A.phit, plo, phi, c);
        const uint64_t qi = A.q0 + P / (E + 1);
        const uint32_t j = uint32_t(P % (E + 1));
        const uint64_t a = A.qoff[qi], m = A.qoff[qi + 1] - a;
        const int64_t D = int64_t(A.pos[c]) - int64_t(piece_start(m, E, j));
        bool run = A.qstat[qi] == KMX_Q_OK && D + int64_t(E) >= 0;
        // a diagonal that an earlier piece of the query names too is left to that piece
        for (uint32_t jj = 0; jj < j && run; ++jj) {
            const int64_t t = D + int64_t(piece_start(m, E, jj));
            if (t < 0) continue;
            const uint64_t lo = A.phit[P - j + jj], hi = A.phit[P - j + jj + 1];
            const uint64_t at = lower_u32(A.pos, lo, hi, uint32_t(t));
            if (at < hi && A.pos[at] == uint32_t(t)) run = false;
        }
        if (run) {
            const uint64_t* __restrict__ qw = A.qwords + a / L + qi;
            uint32_t cell[NB];
#pragma unroll
            for (uint32_t r = 0; r < NB; ++r) cell[r] = int64_t(m) + D + int64_t(r) - int64_t(2 * E) <= n ? 0u : kEditInf;
            bool alive = true;
            for (uint64_t i = m; alive && i-- > 0;) {
                const int64_t base = int64_t(i) + D - int64_t(2 * E);
                uint64_t f0, f1;
                window_neq<W, NB>(A.text, base, A.n, query_letter<W>(qw, i), f0, f1);
                const int64_t lim = n - base;              // cell r is inside the text (t <= n) when r <= lim
                uint32_t row_min = kEditInf;
#pragma unroll
                for (int r = int(NB) - 1; r >= 0; --r) {
                    uint32_t v = cell[r] + neq_at<W>(f0, f1, uint32_t(r));
                    if (r > 0) v = min(v, cell[r - 1] + 1);
                    if (r < int(NB) - 1) v = min(v, cell[r + 1] + 1);
                    v = min(v, kEditInf);
                    if (int64_t(r) > lim) v = kEditInf;
                    cell[r] = v;
                    row_min = min(row_min, v);
                }
                alive = row_min <= E;
            }
            if (alive) {
                out = 0;
#pragma unroll
                for (uint32_t k = 0; k <= 2 * E; ++k) {
                    const bool hit = D - int64_t(E) + int64_t(k) >= 0 && cell[E + k] <= E;
                    out |= (hit ? cell[E + k] : kEditNone) << (3 * k);
                    kept_here += hit;
                }
            }
        }
        A.keep[c] = out;
    }
    if (kept_here) atomicAdd(&s_kept, kept_here);
    __syncthreads();
    if (threadIdx.x == 0) A.bcount[blockIdx.x] = s_kept;
}

// The surviving starts as (query within the chunk << pbits | p, distance) pairs, block b from bscan[b] in any order (they are
// sorted next).
__global__ __launch_bounds__(kBlock) void k_edit_emit(EditArgs A, const uint64_t* __restrict__ bscan, uint32_t pbits,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_at;
    const uint64_t c0 = uint64_t(blockIdx.x) * kVerifySpan;
    const uint64_t c_end = min(c0 + kVerifySpan, A.n_cand);
    if (A.bcount[blockIdx.x] == 0) return;                      // (block-uniform)
    if (threadIdx.x == 0) {
        s_range[0] = piece_of(A.phit, 0, A.np, c0);
        s_range[1] = piece_of(A.phit, s_range[0], A.np, c_end - 1) + 1;
        s_at = 0;
    }
    __syncthreads();
    const uint32_t e = A.e;
    const uint64_t base = bscan[blockIdx.x];
    for (uint32_t it = 0; it < kVerifyCpt; ++it) {
        const uint64_t c = c0 + uint64_t(it) * kBlock + threadIdx.x;
        if (c >= c_end) break;
        const uint32_t k3 = A.keep[c];
        uint32_t cnt = 0;
        for (uint32_t k = 0; k <= 2 * e; ++k) cnt += ((k3 >> (3 * k)) & 7u) != kEditNone;
        if (!cnt) continue;
        const uint64_t P = piece_of(A.phit, s_range[0], s_range[1], c);
        const uint64_t ql = P / (e + 1), qi = A.q0 + ql;
        const uint64_t m = A.qoff[qi + 1] - A.qoff[qi];
        const int64_t D = int64_t(A.pos[c]) - int64_t(piece_start(m, e, uint32_t(P % (e + 1))));
        uint64_t at = base + atomicAdd(&s_at, cnt);
        for (uint32_t k = 0; k <= 2 * e; ++k) {
            const uint32_t d = (k3 >> (3 * k)) & 7u;
            if (d == kEditNone) continue;
            keys[at] = (ql << pbits) | uint64_t(D - int64_t(e) + int64_t(k));
            vals[at] = d;
            ++at;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_edit_heads(const uint64_t* __restrict__ keys, uint64_t n_s, uint32_t* __restrict__ head)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n_s) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// the first of every run of equal keys (equal keys carry equal distances: d(p) does not depend on the diagonal that found it)
__global__ __launch_bounds__(kBlock) void k_edit_unique(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        const uint32_t* __restrict__ head, const uint64_t* __restrict__ rank, uint64_t n_s,
                                                        uint32_t pbits, uint64_t* __restrict__ ukeys, uint32_t* __restrict__ out_pos,
                                                        uint8_t* __restrict__ out_d)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_s || !head[i]) return;
    const uint64_t u = rank[i], key = keys[i];
    ukeys[u] = key;
    out_pos[u] = uint32_t(key & ((uint64_t(1) << pbits) - 1));
    out_d[u] = uint8_t(vals[i]);
}

// hit_off of the chunk's queries: the first distinct key of each
__global__ __launch_bounds__(kBlock) void k_edit_hit_off(const uint64_t* __restrict__ ukeys, uint64_t n_u, uint64_t nq, uint32_t pbits,
                                                         uint64_t* __restrict__ hit_off)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i > nq) return;
    uint64_t lo = 0, hi = n_u;
    const uint64_t x = i << pbits;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ukeys[mid] < x) lo = mid + 1; else hi = mid;
    }
    hit_off[i] = lo;
}

// One thread per reported start p: G[i][c] = distance of q[0, i) to text[p, p + c) on the diagonals c - i = -E .. E (cell r:
// c = i + r - E), updated in place from the first cell to the last; of the cells of row m that hold d(p), the one nearest to
// the main diagonal gives the length, the shorter of two equally near.
template <uint32_t E, uint32_t W>
__global__ __launch_bounds__(kBlock) void k_edit_lengths(const uint64_t* __restrict__ ukeys, const uint8_t* __restrict__ out_d, uint64_t n_u,
                                                         uint32_t pbits, EditArgs A, uint32_t* __restrict__ out_len)
{
    constexpr uint32_t NB = 2 * E + 1, L = 64 / W;
    const uint64_t u = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (u >= n_u) return;
    const uint64_t key = ukeys[u];
    const uint64_t qi = A.q0 + (key >> pbits);
    const int64_t p = int64_t(key & ((uint64_t(1) << pbits) - 1)), n = int64_t(A.n);
    const uint64_t a = A.qoff[qi], m = A.qoff[qi + 1] - a;
    const uint64_t* __restrict__ qw = A.qwords + a / L + qi;
    const uint32_t d = out_d[u];
    uint32_t cell[NB];
#pragma unroll
    for (uint32_t r = 0; r < NB; ++r) cell[r] = (r >= E && p + int64_t(r - E) <= n) ? r - E : kEditInf;
    for (uint64_t i = 1; i <= m; ++i) {
        uint64_t f0, f1;
        window_neq<W, NB>(A.text, p + int64_t(i) - int64_t(E) - 1, A.n, query_letter<W>(qw, i - 1), f0, f1);
        const int64_t lim = n - p - int64_t(i) + int64_t(E);      // cell r ends inside the text (p + c <= n) when r <= lim
#pragma unroll
        for (uint32_t r = 0; r < NB; ++r) {
            uint32_t v = cell[r] + neq_at<W>(f0, f1, r);
            if (r + 1 < NB) v = min(v, cell[r + 1] + 1);
            if (r > 0) v = min(v, cell[r - 1] + 1);
            v = min(v, kEditInf);
            if (int64_t(r) > lim || i + r < E) v = kEditInf;       // (c < 0: no such cell)
            cell[r] = v;
        }
    }
    uint32_t len = 0;                                              // (d(p) is on row m: 0 is never written)
#pragma unroll
    for (int k = int(E); k >= 1; --k) {
        if (cell[E + k] == d) len = uint32_t(m) + k;
        if (cell[E - k] == d) len = uint32_t(m) - k;
    }
    if (cell[E] == d) len = uint32_t(m);
    out_len[u] = len;
}

template <template <uint32_t, uint32_t> class F, typename... Args>
static void edit_dispatch(uint32_t e, uint32_t w, Args&&... args)
{
    switch (e * 16 + w) {
    case 0 * 16 + 2: F<0, 2>::launch(args...); break;
    case 0 * 16 + 4: F<0, 4>::launch(args...); break;
    case 0 * 16 + 8: F<0, 8>::launch(args...); break;
    case 1 * 16 + 2: F<1, 2>::launch(args...); break;
    case 1 * 16 + 4: F<1, 4>::launch(args...); break;
    case 1 * 16 + 8: F<1, 8>::launch(args...); break;
    case 2 * 16 + 2: F<2, 2>::launch(args...); break;
    case 2 * 16 + 4: F<2, 4>::launch(args...); break;
    case 2 * 16 + 8: F<2, 8>::launch(args...); break;
    case 3 * 16 + 2: F<3, 2>::launch(args...); break;
    case 3 * 16 + 4: F<3, 4>::launch(args...); break;
    default: F<3, 8>::launch(args...); break;
    }
}
template <uint32_t E, uint32_t W> struct LaunchEditVerify {
    static void launch(hipStream_t s, unsigned nb, const EditArgs& A) { hipLaunchKernelGGL((k_edit_verify<E, W>), dim3(nb), dim3(kBlock), 0, s, A); }
};
template <uint32_t E, uint32_t W> struct LaunchEditLengths {
    static void launch(hipStream_t s, const uint64_t* ukeys, const uint8_t* out_d, uint64_t n_u, uint32_t pbits, const EditArgs& A, uint32_t* out_len)
    {
        hipLaunchKernelGGL((k_edit_lengths<E, W>), dim3(grid_for(n_u, kBlock)), dim3(kBlock), 0, s, ukeys, out_d, n_u, pbits, A, out_len);
    }
};

// ------------------------------------------------------------------------------------------------------------------------
// both strands (kmx_search_approx_strands): every query goes through the pipeline above twice, as itself and as its reverse
// complement rc(q)[r] = comp[q[m - 1 - r]], inside ONE internal batch of twice the queries: internal query 2i is q_i, 2i + 1
// is rc(q_i), their letters side by side at 2 * qoff[i] and 2 * qoff[i] + m.  The uploaded letters are read once
// (k_strand_prep), the two hit lists of a pair are interleaved by (position, strand) on the device (k_strand_merge).

// One thread per public query: what k_approx_prep does, for both internal queries of the pair.  The statuses a query takes
// from itself alone are those of its reverse complement too (the same length; comp maps the alphabet onto itself).
__global__ __launch_bounds__(kBlock) void k_strand_prep(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ qoff, uint64_t nq,
                                                        const uint8_t* __restrict__ comp, uint32_t sigma, uint32_t e, uint32_t range,
                                                        uint32_t w, uint8_t* __restrict__ qr, uint64_t* __restrict__ iqoff,
                                                        uint64_t* __restrict__ poff, uint8_t* __restrict__ qstat,
                                                        uint64_t* __restrict__ qwords)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= nq) return;
    const uint64_t a = qoff[i], m = qoff[i + 1] - a;
    const uint64_t a0 = 2 * a, a1 = a0 + m;
    const uint32_t L = 64 / w;
    uint8_t st = KMX_Q_OK;
    if (m == 0) st = KMX_Q_EMPTY_QUERY;
    else if (m <= e) st = KMX_Q_TOO_SHORT;
    else if ((m + e) / (e + 1) >= range) st = KMX_Q_TOO_LONG;
    if (st == KMX_Q_OK) {
        uint64_t* qw0 = qwords + a0 / L + 2 * i;
        uint64_t* qw1 = qwords + a1 / L + 2 * i + 1;
        uint64_t v0 = 0, v1 = 0;
        for (uint64_t r = 0; r < m; ++r) {
            const uint32_t c0 = raw[a + r], cb = raw[a + m - 1 - r];
            const uint32_t c1 = comp[cb];
            if (c0 >= sigma) st = KMX_Q_BAD_RANK;
            qr[a0 + r] = uint8_t(c0);
            qr[a1 + r] = uint8_t(c1);
            v0 |= uint64_t(c0 & ((1u << w) - 1)) << ((r % L) * w);
            v1 |= uint64_t(c1 & ((1u << w) - 1)) << ((r % L) * w);
            if (r % L == L - 1 || r + 1 == m) { qw0[r / L] = v0; qw1[r / L] = v1; v0 = 0; v1 = 0; }
        }
    }
    qstat[2 * i] = st;
    qstat[2 * i + 1] = st;
    iqoff[2 * i] = a0;
    iqoff[2 * i + 1] = a1;
    for (uint32_t j = 0; j <= e; ++j) {
        const uint64_t o = piece_start(m, e, j);
        poff[2 * i * (e + 1) + j] = a0 + o;
        poff[(2 * i + 1) * (e + 1) + j] = a1 + o;
    }
    if (i + 1 == nq) {
        iqoff[2 * nq] = 2 * qoff[nq];
        poff[2 * nq * (e + 1)] = 2 * qoff[nq];
    }
    if (st != KMX_Q_OK)                                   // (no letter of the pair costs the exact search anything)
        for (uint64_t r = 0; r < 2 * m; ++r) qr[a0 + r] = sigma < 256 ? uint8_t(255) : raw[a + r % m];
}

// A pair is served only if both strands are: the forward strand's status unless that is KMX_Q_OK, else the reverse strand's.
// Runs behind k_approx_status and in front of the verification, which skips every query that is not KMX_Q_OK.
__global__ __launch_bounds__(kBlock) void k_strand_status(uint8_t* __restrict__ qstat, uint64_t n_pairs, uint8_t* __restrict__ pair_stat)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_pairs) return;
    const uint8_t s0 = qstat[2 * i], s1 = qstat[2 * i + 1];
    const uint8_t s = s0 != KMX_Q_OK ? s0 : s1;
    qstat[2 * i] = s;
    qstat[2 * i + 1] = s;
    pair_stat[i] = s;
}

// first index in [lo, hi) with a[i] > x
__device__ __forceinline__ uint64_t upper_u32(const uint32_t* __restrict__ a, uint64_t lo, uint64_t hi, uint32_t x)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One thread per internal hit t of internal query I (ihit_off[I] <= t < ihit_off[I + 1]): it goes to the pair's first slot +
// its rank in its own list + the hits of the partner list in front of it in (position, strand) order: those below its
// position for a forward hit, those at or below it for a reverse hit.  Both lists are strictly ascending.  Threads
// 0 .. n_pairs also write the public hit_off (= the internal one at even indexes).  len_in is NULL for Hamming results.
__global__ __launch_bounds__(kBlock) void k_strand_merge(const uint64_t* __restrict__ ihit_off, uint64_t n_pairs, uint64_t n_s,
                                                         const uint32_t* __restrict__ pos_in, const uint8_t* __restrict__ d_in,
                                                         const uint32_t* __restrict__ len_in, uint32_t* __restrict__ pos_out,
                                                         uint8_t* __restrict__ d_out, uint32_t* __restrict__ len_out,
                                                         uint8_t* __restrict__ strand_out, uint64_t* __restrict__ hit_off)
{
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t <= n_pairs) hit_off[t] = ihit_off[2 * t];
    if (t >= n_s) return;
    const uint64_t I = piece_of(ihit_off, 0, 2 * n_pairs, t);
    const uint64_t lo = ihit_off[I ^ 1], hi = ihit_off[(I ^ 1) + 1];
    const uint32_t p = pos_in[t];
    const uint64_t before = ((I & 1) ? upper_u32(pos_in, lo, hi, p) : lower_u32(pos_in, lo, hi, p)) - lo;
    const uint64_t dest = ihit_off[I & ~uint64_t(1)] + (t - ihit_off[I]) + before;
    pos_out[dest] = p;
    d_out[dest] = d_in[t];
    if (len_in) len_out[dest] = len_in[t];
    strand_out[dest] = uint8_t(I & 1);
}

// ------------------------------------------------------------------------------------------------------------------------
// reporting (kmx_search_approx_opts with KMX_APPROX_LOCI, KMX_APPROX_BEST or max_hits): the chunk's final hit lists, ordered by
// (position, strand), are filtered on the device in front of the copy to the host.  A hit is a survivor unless the LOCI rule
// removes it (a rule about the neighbours it has in the unfiltered list, so one pass decides it); the survivors of a query are
// counted per distance (four strata), from which one thread per query derives found[q], the lowest stratum kept, the
// threshold stratum t* and the quota left in it; only under a cap do the hits need ranks (a scan of "survivor of its query's
// t*"); a scan of the keep flags then places every kept hit and gives the new hit_off.

struct ReportArgs {
    const uint64_t* hit_off;  // [nq + 1] the chunk's public lists
    uint64_t nq, n_s;
    const uint32_t* pos;      // [n_s]
    const uint8_t* d;         // [n_s] mismatches or distances, <= KMX_APPROX_MAX_SUBST
    const uint8_t* strand;    // [n_s], NULL for one strand
    uint32_t e, loci, best, max_hits;
};

constexpr uint8_t kReportDead = 0xFF;
constexpr uint32_t kStrata = KMX_APPROX_MAX_SUBST + 1;

// One thread per hit: its query (the block's range of queries first, as the verify kernels find their pieces), the LOCI rule
// against the neighbours within e letters on its strand (one strand: at most e list neighbours per side, both: 2e + 1), and a
// survivor's count into its query's stratum.  A neighbour to the left suppresses with d' <= d, one to the right with d' < d.
__global__ __launch_bounds__(kBlock) void k_report_mark(ReportArgs A, uint32_t* __restrict__ hq, uint8_t* __restrict__ code,
                                                        uint32_t* __restrict__ qcnt)
{
    __shared__ uint64_t s_range[2];
    const uint64_t t0 = uint64_t(blockIdx.x) * kBlock, t_end = min(t0 + kBlock, A.n_s);
    if (threadIdx.x == 0) {
        s_range[0] = piece_of(A.hit_off, 0, A.nq, t0);
        s_range[1] = piece_of(A.hit_off, s_range[0], A.nq, t_end - 1) + 1;
    }
    __syncthreads();
    const uint64_t t = t0 + threadIdx.x;
    if (t >= A.n_s) return;
    const uint64_t q = piece_of(A.hit_off, s_range[0], s_range[1], t);
    const uint32_t p = A.pos[t], d = A.d[t], e = A.e;
    bool alive = true;
    if (A.loci && e) {
        const uint64_t a = A.hit_off[q], b = A.hit_off[q + 1];
        const uint8_t s = A.strand ? A.strand[t] : uint8_t(0);
        for (uint64_t u = t; alive && u-- > a;) {
            const uint32_t p2 = A.pos[u];
            if (p - p2 > e) break;
            if (p2 != p && (!A.strand || A.strand[u] == s) && A.d[u] <= d) alive = false;
        }
        for (uint64_t u = t + 1; alive && u < b; ++u) {
            const uint32_t p2 = A.pos[u];
            if (p2 - p > e) break;
            if (p2 != p && (!A.strand || A.strand[u] == s) && A.d[u] < d) alive = false;
        }
    }
    hq[t] = uint32_t(q);
    code[t] = alive ? uint8_t(d) : kReportDead;
    if (alive) atomicAdd(&qcnt[q * kStrata + d], 1u);
}

// rule word of a query: quota in the threshold stratum (bits 0 .. 31), the threshold stratum t* (32 .. 39), the lowest stratum
// kept (40 .. 47).  A survivor at distance d is kept when lo <= d < t*, or d == t* and its rank among the query's survivors
// of t* is below the quota.
__device__ __forceinline__ uint32_t rule_quota(uint64_t r) { return uint32_t(r); }
__device__ __forceinline__ uint32_t rule_tstar(uint64_t r) { return uint32_t(r >> 32) & 0xFFu; }
__device__ __forceinline__ uint32_t rule_lo(uint64_t r) { return uint32_t(r >> 40) & 0xFFu; }

// One thread per query: found[q] = survivors after LOCI and BEST, and the query's rule word.
__global__ __launch_bounds__(kBlock) void k_report_query(const uint32_t* __restrict__ qcnt, uint64_t nq, uint32_t best, uint32_t max_hits,
                                                         uint64_t* __restrict__ found, uint64_t* __restrict__ rule)
{
    const uint64_t q = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (q >= nq) return;
    uint32_t c[kStrata];
#pragma unroll
    for (uint32_t d = 0; d < kStrata; ++d) c[d] = qcnt[q * kStrata + d];
    uint32_t lo = 0, hi = kStrata - 1;
    if (best) {
        while (lo < hi && c[lo] == 0) ++lo;
        hi = lo;
    }
    uint64_t n = 0;
    for (uint32_t d = lo; d <= hi; ++d) n += c[d];
    uint32_t tstar = hi, quota = 0xFFFFFFFFu;
    if (max_hits && n > max_hits) {
        uint32_t acc = 0;
        for (uint32_t d = lo; d <= hi; ++d) {
            if (acc + c[d] >= max_hits) { tstar = d; quota = max_hits - acc; break; }
            acc += c[d];
        }
    }
    found[q] = n;
    rule[q] = uint64_t(quota) | (uint64_t(tstar) << 32) | (uint64_t(lo) << 40);
}

// ind[t] = 1 for a survivor of its query's threshold stratum (the only hits whose rank matters)
__global__ __launch_bounds__(kBlock) void k_report_ind(const uint8_t* __restrict__ code, const uint32_t* __restrict__ hq,
                                                       const uint64_t* __restrict__ rule, uint64_t n_s, uint32_t* __restrict__ ind)
{
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t < n_s) ind[t] = code[t] == rule_tstar(rule[hq[t]]) ? 1u : 0u;
}

// keep[t]; rscan is the exclusive scan of ind (NULL without a cap: no quota is finite)
__global__ __launch_bounds__(kBlock) void k_report_keep(const uint8_t* __restrict__ code, const uint32_t* __restrict__ hq,
                                                        const uint64_t* __restrict__ rule, const uint64_t* __restrict__ hit_off,
                                                        const uint64_t* __restrict__ rscan, uint64_t n_s, uint32_t* __restrict__ keep)
{
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_s) return;
    const uint32_t d = code[t], q = hq[t];
    const uint64_t r = rule[q];
    bool k = d != kReportDead && d >= rule_lo(r) && d <= rule_tstar(r);
    if (k && rscan && d == rule_tstar(r)) k = rscan[t] - rscan[hit_off[q]] < rule_quota(r);
    keep[t] = k ? 1u : 0u;
}

// dest is the exclusive scan of keep (dest[n_s] = the hits kept): every kept hit to its slot, threads 0 .. nq the new hit_off.
__global__ __launch_bounds__(kBlock) void k_report_compact(ReportArgs A, const uint32_t* __restrict__ len_in, const uint32_t* __restrict__ keep,
                                                           const uint64_t* __restrict__ dest, uint32_t* __restrict__ pos_out,
                                                           uint8_t* __restrict__ d_out, uint32_t* __restrict__ len_out,
                                                           uint8_t* __restrict__ strand_out, uint64_t* __restrict__ hit_off_out)
{
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t <= A.nq) hit_off_out[t] = dest[A.hit_off[t]];
    if (t >= A.n_s || !keep[t]) return;
    const uint64_t at = dest[t];
    pos_out[at] = A.pos[t];
    d_out[at] = A.d[t];
    if (len_in) len_out[at] = len_in[t];
    if (A.strand) strand_out[at] = A.strand[t];
}

// ------------------------------------------------------------------------------------------------------------------------
// host side

void kmx::packed_text_release(PackedText* t)
{
    if (!t) return;
    std::lock_guard<std::mutex> lock(t->mu);
    if (t->d_words) (void)hipFree(t->d_words);
    t->d_words = nullptr;
    t->ready = false;
}

// Derives the replica's packed text (once; retried after a failure).  The index's device is current.
kmx_status kmx::ensure_text(const kmx::IndexAccess& A, hipStream_t s)
{
    kmx::PackedText& T = *A.text;
    std::lock_guard<std::mutex> lock(T.mu);
    if (T.ready) return KMX_OK;
    const KmxIndexDev& h = *A.h;
    uint32_t el = 0;                                     // the element with the fewest groups: the shortest binary searches
    for (uint32_t i = 1; i < h.n_ks; ++i) {
        const uint64_t gi = h.elems[i].table_kind == KMX_TABLE_DENSE ? h.elems[i].n_keys : h.elems[i].n_ukeys;
        const uint64_t ge = h.elems[el].table_kind == KMX_TABLE_DENSE ? h.elems[el].n_keys : h.elems[el].n_ukeys;
        if (gi < ge) el = i;
    }
    const KmxElemDev& E = h.elems[el];
    const uint64_t n = A.n;
    const uint32_t w = bits_per_letter(A.sigma);
    const uint64_t n_words = (n * w + 63) / 64 + KMX_TEXT_PAD_WORDS;
    Buf t8;
    TRY_HIP(t8.ensure(n + 64));
    uint64_t* words = nullptr;
    TRY_HIP(hipMalloc(&words, n_words * 8));
    auto fail_free = [&](hipError_t e) {
        (void)hipFree(words);
        (void)hipGetLastError();
        return kmx::set_error(e == hipErrorOutOfMemory ? KMX_ERR_OUT_OF_MEMORY : KMX_ERR_HIP, std::string("kmx_index_text: ") + hipGetErrorString(e));
    };
    const uint64_t n_groups = E.table_kind == KMX_TABLE_DENSE ? E.n_keys : uint64_t(E.n_ukeys);
    hipLaunchKernelGGL(k_text_scatter, dim3(std::min<unsigned>(grid_for(E.npos, kBlock), 65536u)), dim3(kBlock), 0, s, h.arena + E.arena_base, E.offs,
                       E.table_kind == KMX_TABLE_DENSE ? (const uint64_t*)nullptr : E.ukeys, n_groups, E.npos, h.pw[E.k - 1], n, t8.as<uint8_t>());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(t8.as<uint8_t>() + (n - h.kmax), h.tail, h.kmax, hipMemcpyDeviceToDevice, s);   // the last kmax letters
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_text_pack, dim3(std::min<unsigned>(grid_for(n_words, kBlock), 65536u)), dim3(kBlock), 0, s, t8.as<uint8_t>(), n, w, n_words, words);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_free(e);
    T.d_words = words;
    T.n_words = n_words;
    T.w = w;
    T.ready = true;
    return KMX_OK;
}

namespace {
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
// the exact-search result of the pieces: its last search ran on stream `s`, which is drained before the result goes back to
// the index's pool, so that kmx_result_free need not wait for the whole device
struct ResultGuard {
    kmx_result* r = nullptr;
    hipStream_t s = nullptr;
    ~ResultGuard()
    {
        if (!r) return;
        if (s && hipStreamSynchronize(s) == hipSuccess) kmx::result_quiesced(r);
        else (void)hipGetLastError();
        kmx_result_free(r);
    }
};

// a launch and its launch error; AX_LAUNCH: a kernel on `blocks` blocks of kBlock threads on stream s
#define AX_RUN(...) do { __VA_ARGS__; TRY_HIP(hipGetLastError()); } while (0)
#define AX_LAUNCH(kernel, blocks, s, ...) AX_RUN(hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, s, __VA_ARGS__))

// One chunk's hit lists on the device, as one stage hands them to the next: the statuses of its nq queries, hit_off[nq + 1],
// n_hits positions and distances (Hamming: mismatches); len is NULL unless KMX_APPROX_EDIT, strand is NULL for one strand.
struct ChunkLists {
    uint64_t nq = 0, n_hits = 0;
    const uint8_t* stat = nullptr;
    const uint64_t* hit_off = nullptr;
    const uint32_t* pos = nullptr;
    const uint8_t* dist = nullptr;
    const uint32_t* len = nullptr;
    const uint8_t* strand = nullptr;
};
struct PrepBufs {
    std::vector<uint64_t> loc;                           // the chunk's query offsets on the host, rebased to the chunk
    Buf qr, qoff, poff, qstat, qwords, qcand, raw, d_loc, comp, pair_stat;      // (the last four: both strands only)
};
struct SubstBufs { Buf keep, bcount, bsum, bscan, total, spos, spiece, smm, hit_off, opos, omm; };
struct EditBufs { Buf keep, bcount, bsum, bscan, total, ka, va, kb, vb, ukeys, hit_off, opos, od, olen; };
struct StrandBufs { Buf off, pos, d, len, strand; };
struct ReportBufs { Buf hq, code, qcnt, rule, found, flag, rscan, dest, bsum, total, off, pos, d, len, strand; };
// what kmx_search_approx_opts asks for beyond the older entry points (they pass a default-constructed one)
struct ReportOpts {
    bool api = false, loci = false, best = false;
    uint32_t max_hits = 0;
    bool on() const { return loci || best || max_hits != 0; }
};
inline uint32_t bit_width(uint64_t x) { uint32_t b = 0; while (x) { ++b; x >>= 1; } return b; }
} // namespace

// *n <- the total a scan left on the device; the stream is drained
static kmx_status read_total(hipStream_t s, const Buf& d_total, PinnedArr& h_total, uint64_t* n)
{
    TRY_HIP(hipMemcpyAsync(h_total.p, d_total.p, 8, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    *n = h_total.as<uint64_t>()[0];
    return KMX_OK;
}

static kmx_status grow_pinned(PinnedArr& a, size_t bytes, const std::string& who)
{
    return a.grow(bytes) ? KMX_OK : kmx::set_error(KMX_ERR_OUT_OF_MEMORY, who + "page-locked host memory");
}

static kmx_status check_queries(const std::string& who, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq)
{
    if (nq && !qoff) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "NULL query offsets");
    if (nq && qoff[0] != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "qoff[0] must be 0");
    for (uint64_t i = 0; i < nq; ++i)
        if (qoff[i + 1] < qoff[i]) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "qoff must be non-decreasing");
    if (nq && !qranks && qoff[nq] != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "NULL query letters");
    return KMX_OK;
}

// comp[256] <- the complement table, the identity outside the alphabet (letters there: the pair is KMX_Q_BAD_RANK)
kmx_status kmx::check_complement(const std::string& who, const uint8_t* complement, uint32_t sigma, uint8_t* comp)
{
    for (uint32_t r = 0; r < 256; ++r) comp[r] = uint8_t(r);
    for (uint32_t r = 0; r < sigma && r < 256; ++r)                   // every entry's range first: an entry outside the alphabet is
        if (complement[r] >= sigma)                                   // reported as that, whichever rank maps to it
            return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "complement[" + std::to_string(r) + "] is outside the alphabet");
    for (uint32_t r = 0; r < sigma && r < 256; ++r) {
        const uint32_t c = complement[r];
        if (complement[c] != r)
            return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the complement table is not an involution at rank " + std::to_string(r));
        comp[r] = uint8_t(c);
    }
    return KMX_OK;
}

// The letters of queries [Q0, Q1) (a copy the prep kernel may overwrite) and their offsets, rebased, to the device; from them
// the chunk's internal queries (S = 2: every query and its reverse complement), their pieces, statuses and packed words.
static kmx_status prep_chunk(hipStream_t s, const kmx::IndexAccess& A, const uint8_t* qranks, const uint64_t* qoff, uint64_t Q0, uint64_t Q1,
                             uint32_t S, uint32_t e, PrepBufs& B)
{
    const uint64_t nqc = Q1 - Q0, nqi = nqc * S, l0 = qoff[Q0], n_letters = qoff[Q1] - l0;
    const uint32_t E1 = e + 1, w = A.text->w, L = 64 / w;
    B.loc.resize(nqc + 1);
    for (uint64_t i = 0; i <= nqc; ++i) B.loc[i] = qoff[Q0 + i] - l0;
    TRY_HIP(B.qr.ensure(n_letters * S + 64));
    TRY_HIP(B.qoff.ensure((nqi + 1) * 8));
    TRY_HIP(B.poff.ensure((nqi * E1 + 1) * 8));
    TRY_HIP(B.qstat.ensure(nqi + 16));
    TRY_HIP(B.qwords.ensure((n_letters * S / L + nqi + 2) * 8));
    TRY_HIP(B.qcand.ensure((nqc + 1) * 8));
    if (S == 2) {
        TRY_HIP(B.raw.ensure(n_letters + 64));
        TRY_HIP(B.d_loc.ensure((nqc + 1) * 8));
        TRY_HIP(B.pair_stat.ensure(nqc + 16));
    }
    const Buf &letters = S == 1 ? B.qr : B.raw, &offs = S == 1 ? B.qoff : B.d_loc;      // what the prep kernel reads
    if (n_letters) TRY_HIP(hipMemcpyAsync(letters.p, qranks + l0, n_letters, hipMemcpyHostToDevice, s));
    TRY_HIP(hipMemcpyAsync(offs.p, B.loc.data(), (nqc + 1) * 8, hipMemcpyHostToDevice, s));
    if (S == 1)
        AX_LAUNCH(k_approx_prep, grid_for(nqc, kBlock), s, B.qr.as<uint8_t>(), B.qoff.as<uint64_t>(), nqc, A.sigma, e, A.range, w,
                  B.poff.as<uint64_t>(), B.qstat.as<uint8_t>(), B.qwords.as<uint64_t>());
    else
        AX_LAUNCH(k_strand_prep, grid_for(nqc, kBlock), s, B.raw.as<uint8_t>(), B.d_loc.as<uint64_t>(), nqc, B.comp.as<uint8_t>(), A.sigma, e, A.range,
                  w, B.qr.as<uint8_t>(), B.qoff.as<uint64_t>(), B.poff.as<uint64_t>(), B.qstat.as<uint8_t>(), B.qwords.as<uint64_t>());
    return KMX_OK;
}

// a chunk without a hit: L <- hit_off all zero
static kmx_status no_hits(hipStream_t s, const Buf& hit_off, ChunkLists& L)
{
    TRY_HIP(hipMemsetAsync(hit_off.p, 0, (L.nq + 1) * 8, s));
    L = ChunkLists{L.nq, 0, L.stat, hit_off.as<uint64_t>()};
    return KMX_OK;
}

// The substitution path of one chunk behind the piece search: L <- hit_off, positions and mismatches of its L.nq queries.
static kmx_status subst_chunk(hipStream_t s, VerifyArgs V, SubstBufs& B, PinnedArr& h_total, ChunkLists& L)
{
    TRY_HIP(B.hit_off.ensure((L.nq + 1) * 8));
    if (!V.n_cand) return no_hits(s, B.hit_off, L);
    const uint64_t nb = (V.n_cand + kVerifySpan - 1) / kVerifySpan;
    TRY_HIP(B.keep.ensure(V.n_cand));
    TRY_HIP(B.bcount.ensure(nb * 4 + 16));
    TRY_HIP(B.bsum.ensure(kmx::scan_blocks(nb) * 8 + 16));
    TRY_HIP(B.bscan.ensure((nb + 1) * 8));
    TRY_HIP(B.total.ensure(16));
    V.keep = B.keep.as<uint8_t>();
    V.bcount = B.bcount.as<uint32_t>();
    AX_LAUNCH(k_approx_verify, unsigned(nb), s, V);
    AX_RUN(kmx::launch_scan(s, V.bcount, nb, B.bsum.as<uint64_t>(), B.bscan.as<uint64_t>(), B.total.as<unsigned long long>()));
    uint64_t n_s = 0;
    TRY_KMX(read_total(s, B.total, h_total, &n_s));
    if (!n_s) return no_hits(s, B.hit_off, L);
    TRY_HIP(B.spos.ensure(n_s * 4));
    TRY_HIP(B.spiece.ensure(n_s * 4));
    TRY_HIP(B.smm.ensure(n_s));
    TRY_HIP(B.opos.ensure(n_s * 4));
    TRY_HIP(B.omm.ensure(n_s));
    AX_LAUNCH(k_approx_compact, unsigned(nb), s, V, B.bscan.as<uint64_t>(), B.spos.as<uint32_t>(), B.spiece.as<uint32_t>(), B.smm.as<uint8_t>());
    AX_LAUNCH(k_approx_merge, grid_for(n_s, kBlock), s, B.spos.as<uint32_t>(), B.spiece.as<uint32_t>(), B.smm.as<uint8_t>(), n_s, V.e,
              B.opos.as<uint32_t>(), B.omm.as<uint8_t>());
    AX_LAUNCH(k_approx_hit_off, grid_for(L.nq + 1, kBlock), s, B.spiece.as<uint32_t>(), n_s, L.nq, V.e, B.hit_off.as<uint64_t>());
    L = ChunkLists{L.nq, n_s, L.stat, B.hit_off.as<uint64_t>(), B.opos.as<uint32_t>(), B.omm.as<uint8_t>()};
    return KMX_OK;
}

// The edit path of one chunk behind the piece search: L <- hit_off, positions, distances and lengths of its L.nq queries.
static kmx_status edit_chunk(hipStream_t s, EditArgs V, uint32_t w, EditBufs& B, PinnedArr& h_total, ChunkLists& L)
{
    const uint64_t nq = L.nq;
    TRY_HIP(B.hit_off.ensure((nq + 1) * 8));
    if (!V.n_cand) return no_hits(s, B.hit_off, L);
    const uint64_t nb = (V.n_cand + kVerifySpan - 1) / kVerifySpan;
    TRY_HIP(B.keep.ensure(V.n_cand * 4));
    TRY_HIP(B.bcount.ensure(nb * 4 + 16));
    TRY_HIP(B.bsum.ensure(kmx::scan_blocks(nb) * 8 + 16));
    TRY_HIP(B.bscan.ensure((nb + 1) * 8));
    TRY_HIP(B.total.ensure(16));
    V.keep = B.keep.as<uint32_t>();
    V.bcount = B.bcount.as<uint32_t>();
    AX_RUN(edit_dispatch<LaunchEditVerify>(V.e, w, s, unsigned(nb), V));
    AX_RUN(kmx::launch_scan(s, V.bcount, nb, B.bsum.as<uint64_t>(), B.bscan.as<uint64_t>(), B.total.as<unsigned long long>()));
    uint64_t n_s = 0, n_u = 0;
    TRY_KMX(read_total(s, B.total, h_total, &n_s));
    if (!n_s) return no_hits(s, B.hit_off, L);
    const uint32_t pbits = std::max(bit_width(V.n - 1), 1u), key_bits = pbits + bit_width(nq - 1);
    TRY_HIP(B.ka.ensure((n_s + 1) * 8));                                      // (+ 1: whichever pair the sort leaves free takes a scan of
    TRY_HIP(B.kb.ensure((n_s + 1) * 8));                                      //  n_s entries and its total)
    TRY_HIP(B.va.ensure(n_s * 4));
    TRY_HIP(B.vb.ensure(n_s * 4));
    AX_LAUNCH(k_edit_emit, unsigned(nb), s, V, B.bscan.as<uint64_t>(), pbits, B.ka.as<uint64_t>(), B.va.as<uint32_t>());
    bool in_b = false;
    TRY_HIP(kmx::sort_pairs_u64(s, B.ka.as<uint64_t>(), B.va.as<uint32_t>(), B.kb.as<uint64_t>(), B.vb.as<uint32_t>(), n_s, key_bits, &in_b));
    const uint64_t* keys = in_b ? B.kb.as<uint64_t>() : B.ka.as<uint64_t>();
    const uint32_t* vals = in_b ? B.vb.as<uint32_t>() : B.va.as<uint32_t>();
    uint64_t* rank = in_b ? B.ka.as<uint64_t>() : B.kb.as<uint64_t>();        // the other pair of arrays is free again
    uint32_t* head = in_b ? B.va.as<uint32_t>() : B.vb.as<uint32_t>();
    TRY_HIP(B.bsum.ensure(kmx::scan_blocks(n_s) * 8 + 16));
    AX_LAUNCH(k_edit_heads, grid_for(n_s, kBlock), s, keys, n_s, head);
    AX_RUN(kmx::launch_scan(s, head, n_s, B.bsum.as<uint64_t>(), rank, B.total.as<unsigned long long>()));
    TRY_KMX(read_total(s, B.total, h_total, &n_u));                             // (n_u >= 1: the first key heads a run)
    TRY_HIP(B.ukeys.ensure(n_u * 8));
    TRY_HIP(B.opos.ensure(n_u * 4));
    TRY_HIP(B.od.ensure(n_u));
    TRY_HIP(B.olen.ensure(n_u * 4));
    AX_LAUNCH(k_edit_unique, grid_for(n_s, kBlock), s, keys, vals, head, rank, n_s, pbits, B.ukeys.as<uint64_t>(), B.opos.as<uint32_t>(),
              B.od.as<uint8_t>());
    AX_LAUNCH(k_edit_hit_off, grid_for(nq + 1, kBlock), s, B.ukeys.as<uint64_t>(), n_u, nq, pbits, B.hit_off.as<uint64_t>());
    AX_RUN(edit_dispatch<LaunchEditLengths>(V.e, w, s, B.ukeys.as<uint64_t>(), B.od.as<uint8_t>(), n_u, pbits, V, B.olen.as<uint32_t>()));
    L = ChunkLists{nq, n_u, L.stat, B.hit_off.as<uint64_t>(), B.opos.as<uint32_t>(), B.od.as<uint8_t>(), B.olen.as<uint32_t>()};
    return KMX_OK;
}

// Both strands: each pair's two lists of L merged into the pair's one, ordered by (position, strand), with the pairs' statuses.
static kmx_status strand_merge_chunk(hipStream_t s, const uint8_t* pair_stat, StrandBufs& B, ChunkLists& L)
{
    const uint64_t n_pairs = L.nq / 2, n_s = L.n_hits;
    TRY_HIP(B.off.ensure((n_pairs + 1) * 8));
    if (!n_s) TRY_HIP(hipMemsetAsync(B.off.p, 0, (n_pairs + 1) * 8, s));
    if (n_s) {
        TRY_HIP(B.pos.ensure(n_s * 4));
        TRY_HIP(B.d.ensure(n_s));
        TRY_HIP(B.strand.ensure(n_s));
        if (L.len) TRY_HIP(B.len.ensure(n_s * 4));
        AX_LAUNCH(k_strand_merge, grid_for(std::max(n_s, n_pairs + 1), kBlock), s, L.hit_off, n_pairs, n_s, L.pos, L.dist, L.len, B.pos.as<uint32_t>(),
                  B.d.as<uint8_t>(), B.len.as<uint32_t>(), B.strand.as<uint8_t>(), B.off.as<uint64_t>());
    }
    L = ChunkLists{n_pairs, n_s, pair_stat, B.off.as<uint64_t>(), B.pos.as<uint32_t>(), B.d.as<uint8_t>(), L.len ? B.len.as<uint32_t>() : nullptr,
                   B.strand.as<uint8_t>()};
    return KMX_OK;
}

// The reporting stage of one chunk: the lists of L filtered and compacted on the device, found[] of its queries to h_found.
static kmx_status report_chunk(hipStream_t s, const ReportOpts& rep, uint32_t e, ReportBufs& B, PinnedArr& h_total, uint64_t* h_found, ChunkLists& L)
{
    const uint64_t n_s = L.n_hits, nq = L.nq;
    if (!n_s) { std::memset(h_found, 0, nq * 8); return KMX_OK; }
    const ReportArgs P{L.hit_off, nq, n_s, L.pos, L.dist, L.strand, e, rep.loci, rep.best, rep.max_hits};
    TRY_HIP(B.hq.ensure(n_s * 4));
    TRY_HIP(B.code.ensure(n_s));
    TRY_HIP(B.qcnt.ensure(nq * kStrata * 4));
    TRY_HIP(B.rule.ensure(nq * 8));
    TRY_HIP(B.found.ensure(nq * 8));
    TRY_HIP(B.flag.ensure(n_s * 4 + 16));
    TRY_HIP(B.dest.ensure((n_s + 1) * 8));
    TRY_HIP(B.bsum.ensure(kmx::scan_blocks(n_s) * 8 + 16));
    TRY_HIP(B.total.ensure(16));
    TRY_HIP(B.off.ensure((nq + 1) * 8));
    const unsigned hit_blocks = grid_for(n_s, kBlock);
    TRY_HIP(hipMemsetAsync(B.qcnt.p, 0, nq * kStrata * 4, s));
    AX_LAUNCH(k_report_mark, hit_blocks, s, P, B.hq.as<uint32_t>(), B.code.as<uint8_t>(), B.qcnt.as<uint32_t>());
    AX_LAUNCH(k_report_query, grid_for(nq, kBlock), s, B.qcnt.as<uint32_t>(), nq, P.best, P.max_hits, B.found.as<uint64_t>(), B.rule.as<uint64_t>());
    const uint64_t* rscan = nullptr;
    if (P.max_hits) {
        TRY_HIP(B.rscan.ensure((n_s + 1) * 8));
        AX_LAUNCH(k_report_ind, hit_blocks, s, B.code.as<uint8_t>(), B.hq.as<uint32_t>(), B.rule.as<uint64_t>(), n_s, B.flag.as<uint32_t>());
        AX_RUN(kmx::launch_scan(s, B.flag.as<uint32_t>(), n_s, B.bsum.as<uint64_t>(), B.rscan.as<uint64_t>(), B.total.as<unsigned long long>()));
        rscan = B.rscan.as<uint64_t>();
    }
    AX_LAUNCH(k_report_keep, hit_blocks, s, B.code.as<uint8_t>(), B.hq.as<uint32_t>(), B.rule.as<uint64_t>(), P.hit_off, rscan, n_s,
              B.flag.as<uint32_t>());
    AX_RUN(kmx::launch_scan(s, B.flag.as<uint32_t>(), n_s, B.bsum.as<uint64_t>(), B.dest.as<uint64_t>(), B.total.as<unsigned long long>()));
    uint64_t n_keep = 0;
    TRY_KMX(read_total(s, B.total, h_total, &n_keep));
    TRY_HIP(B.pos.ensure(n_keep * 4 + 16));
    TRY_HIP(B.d.ensure(n_keep + 16));
    if (L.len) TRY_HIP(B.len.ensure(n_keep * 4 + 16));
    if (L.strand) TRY_HIP(B.strand.ensure(n_keep + 16));
    AX_LAUNCH(k_report_compact, grid_for(std::max(n_s, nq + 1), kBlock), s, P, L.len, B.flag.as<uint32_t>(), B.dest.as<uint64_t>(), B.pos.as<uint32_t>(),
              B.d.as<uint8_t>(), B.len.as<uint32_t>(), B.strand.as<uint8_t>(), B.off.as<uint64_t>());
    TRY_HIP(hipMemcpyAsync(h_found, B.found.p, nq * 8, hipMemcpyDeviceToHost, s));
    L = ChunkLists{nq, n_keep, L.stat, B.off.as<uint64_t>(), B.pos.as<uint32_t>(), B.d.as<uint8_t>(), L.len ? B.len.as<uint32_t>() : nullptr,
                   L.strand ? B.strand.as<uint8_t>() : nullptr};
    return KMX_OK;
}

// The chunk's lists to the host arrays of R, for the queries from q_at on: the copies, one wait for them, hit_off rebased to the
// hits of the chunks before.
static kmx_status publish_chunk(hipStream_t s, const std::string& who, const ChunkLists& L, uint64_t q_at, kmx_approx_result& R)
{
    const uint64_t h_at = R.n_hits, n = L.n_hits;
    TRY_KMX(grow_pinned(R.positions, (h_at + n) * 4 + 64, who));
    TRY_KMX(grow_pinned(R.mismatches, h_at + n + 64, who));
    if (R.edit) TRY_KMX(grow_pinned(R.lengths, (h_at + n) * 4 + 64, who));
    if (R.strands) TRY_KMX(grow_pinned(R.strand, h_at + n + 64, who));
    uint64_t* ho = R.hit_off.as<uint64_t>() + q_at;          // (ho[0], the previous chunk's end, is rewritten with the same value)
    TRY_HIP(hipMemcpyAsync(ho, L.hit_off, (L.nq + 1) * 8, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipMemcpyAsync(R.status.as<uint8_t>() + q_at, L.stat, L.nq, hipMemcpyDeviceToHost, s));
    if (n) {
        TRY_HIP(hipMemcpyAsync(R.positions.as<uint32_t>() + h_at, L.pos, n * 4, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipMemcpyAsync(R.mismatches.as<uint8_t>() + h_at, L.dist, n, hipMemcpyDeviceToHost, s));
        if (R.edit) TRY_HIP(hipMemcpyAsync(R.lengths.as<uint32_t>() + h_at, L.len, n * 4, hipMemcpyDeviceToHost, s));
        if (R.strands) TRY_HIP(hipMemcpyAsync(R.strand.as<uint8_t>() + h_at, L.strand, n, hipMemcpyDeviceToHost, s));
    }
    TRY_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i <= L.nq; ++i) ho[i] += h_at;
    R.n_hits += n;
    return KMX_OK;
}

extern "C" {

kmx_status kmx_index_text(const kmx_index* index, uint8_t* out_ranks, uint64_t n, uint64_t* packed_bytes)
{
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_index_text: index is NULL");
    const kmx::IndexAccess A = kmx::index_access(index);
    if (out_ranks && n != A.n) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_index_text: n differs from the index's text length");
    DeviceGuard dg;
    TRY_HIP(hipSetDevice(A.device));
    StreamGuard sg;
    TRY_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    TRY_KMX(ensure_text(A, sg.s));
    if (packed_bytes) *packed_bytes = A.text->n_words * 8;
    if (!out_ranks || n == 0) return KMX_OK;
    Buf out;
    TRY_HIP(out.ensure(n));
    AX_LAUNCH(k_text_unpack, std::min<unsigned>(grid_for(n, kBlock), 65536u), sg.s, A.text->d_words, n, A.text->w, out.as<uint8_t>());
    TRY_HIP(hipMemcpyAsync(out_ranks, out.p, n, hipMemcpyDeviceToHost, sg.s));
    TRY_HIP(hipStreamSynchronize(sg.s));
    return KMX_OK;
}

} // extern "C"

// kmx_search_approx (complement == NULL) and kmx_search_approx_strands (the table given): S = 1 or 2 internal queries per
// query of the caller.  `fn` names the entry point in error messages.
static kmx_status approx_search(const char* fn, const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq,
                                uint32_t max_subst, uint32_t flags, const uint8_t* complement, const ReportOpts& rep,
                                kmx_approx_result** out)
{
    const std::string who = std::string(fn) + ": ";
    if (max_subst > KMX_APPROX_MAX_SUBST) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_subst > KMX_APPROX_MAX_SUBST");
    if (flags & ~uint32_t(KMX_APPROX_EDIT)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "unknown flag bits");
    TRY_KMX(check_queries(who, qranks, qoff, nq));
    *out = nullptr;
    const kmx::IndexAccess A = kmx::index_access(index);
    if (A.broken) return kmx::set_error(KMX_ERR_HIP, kmx::kIndexUnusable);
    const uint32_t e = max_subst, E1 = e + 1;
    const uint32_t S = complement ? 2u : 1u;             // internal queries per query (both strands: q and rc(q))
    uint8_t comp[256];
    if (complement) TRY_KMX(kmx::check_complement(who, complement, A.sigma, comp));
    uint64_t budget = kDefaultBudget, max_pieces = kMaxPieces;
    if (const char* env = getenv("KMX_APPROX_CHUNK_CANDIDATES")) { const long long v = atoll(env); if (v > 0) budget = uint64_t(v); }
    if (const char* env = getenv("KMX_APPROX_CHUNK_PIECES")) { const long long v = atoll(env); if (v > 0) max_pieces = std::min(uint64_t(v), kMaxPieces); }
    const bool edit = (flags & KMX_APPROX_EDIT) != 0;
    if (edit) budget = std::max<uint64_t>(budget / (2 * e + 1), 1);      // a piece hit names 2e + 1 starts: each counts against the budget

    DeviceGuard dg;
    TRY_HIP(hipSetDevice(A.device));
    StreamGuard sg;
    TRY_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    hipStream_t s = sg.s;
    TRY_KMX(ensure_text(A, s));
    const uint64_t* text = A.text->d_words;
    const uint32_t w = A.text->w;

    std::unique_ptr<kmx_approx_result> R(new kmx_approx_result());
    R->nq = nq; R->edit = edit; R->strands = complement != nullptr;
    R->opts = rep.api; R->reported = rep.on();
    if (rep.on()) TRY_KMX(grow_pinned(R->found, (nq + 1) * 8, who));
    if (complement) TRY_KMX(grow_pinned(R->strand, 64, who));
    if (edit) TRY_KMX(grow_pinned(R->lengths, 64, who));
    TRY_KMX(grow_pinned(R->hit_off, (nq + 1) * 8, who));
    TRY_KMX(grow_pinned(R->status, nq + 1, who));
    TRY_KMX(grow_pinned(R->positions, 64, who));
    TRY_KMX(grow_pinned(R->mismatches, 64, who));
    R->hit_off.as<uint64_t>()[0] = 0;

    PrepBufs pb;
    SubstBufs sb; EditBufs eb; StrandBufs mb; ReportBufs rb;      // each stage's own
    if (complement) {
        TRY_HIP(pb.comp.ensure(256));
        TRY_HIP(hipMemcpyAsync(pb.comp.p, comp, 256, hipMemcpyHostToDevice, s));
    }
    PinnedArr h_qcand, h_total;
    TRY_KMX(grow_pinned(h_total, 64, who));
    ResultGuard pres{nullptr, s};
    const uint64_t chunk_q = std::max<uint64_t>(max_pieces / (uint64_t(E1) * S), 1);      // (a pair is never split)

    for (uint64_t Q0 = 0; Q0 < nq;) {
        const uint64_t Q1 = std::min(nq, Q0 + chunk_q), nqc = Q1 - Q0;
        TRY_KMX(prep_chunk(s, A, qranks, qoff, Q0, Q1, S, e, pb));
        // candidates per query (both strands: per pair): the pieces through the exact search, counts only
        TRY_KMX(kmx_search_batch_device(index, pb.qr.p, pb.poff.p, nqc * S * E1, KMX_SEARCH_COUNT_ONLY, s, &pres.r));
        const uint64_t* d_phit = nullptr;
        TRY_KMX(kmx_result_view_device(pres.r, &d_phit, nullptr, nullptr));
        AX_LAUNCH(k_approx_query_cands, grid_for(nqc + 1, kBlock), s, d_phit, nqc, S * E1 - 1, pb.qcand.as<uint64_t>());
        TRY_KMX(grow_pinned(h_qcand, (nqc + 1) * 8, who));
        TRY_HIP(hipMemcpyAsync(h_qcand.p, pb.qcand.p, (nqc + 1) * 8, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipStreamSynchronize(s));
        const uint64_t* qc = h_qcand.as<uint64_t>();

        for (uint64_t a = 0; a < nqc;) {
            // the longest run of queries whose candidates fit the budget (at least one query)
            uint64_t b = uint64_t(std::upper_bound(qc + a + 1, qc + nqc + 1, qc[a] + budget) - qc) - 1;
            b = std::max(b, a + 1);
            const uint64_t nqv = (b - a) * S, q0 = a * S, np = nqv * E1;     // the chunk's internal queries [q0, q0 + nqv), their pieces
            R->n_chunks += 1;
            TRY_KMX(kmx_search_batch_device(index, pb.qr.p, pb.poff.as<uint64_t>() + q0 * E1, np, KMX_SEARCH_DEFAULT, s, &pres.r));
            const uint64_t* phit = nullptr; const uint32_t* ppos = nullptr; const uint8_t* pstat = nullptr;
            TRY_KMX(kmx_result_view_device(pres.r, &phit, &ppos, &pstat));
            uint64_t n_cand = 0;
            TRY_KMX(kmx_result_counts(pres.r, nullptr, &n_cand, nullptr, nullptr, nullptr, nullptr));
            R->n_candidates += n_cand;
            AX_LAUNCH(k_approx_status, grid_for(nqv, kBlock), s, pstat, nqv, e, pb.qstat.as<uint8_t>() + q0);
            if (S == 2) AX_LAUNCH(k_strand_status, grid_for(b - a, kBlock), s, pb.qstat.as<uint8_t>() + q0, b - a, pb.pair_stat.as<uint8_t>() + a);
            // the stages: the internal queries' lists, (both strands) each pair's two merged, (reporting) filtered, then to the host
            ChunkLists L{nqv, 0, pb.qstat.as<uint8_t>() + q0};
            const uint64_t* d_qoff = pb.qoff.as<uint64_t>(); const uint8_t* d_qstat = pb.qstat.as<uint8_t>(); const uint64_t* d_qwords = pb.qwords.as<uint64_t>();
            if (edit) TRY_KMX(edit_chunk(s, EditArgs{phit, ppos, n_cand, np, d_qoff, q0, d_qstat, d_qwords, text, A.n, e, nullptr, nullptr}, w, eb, h_total, L));
            else TRY_KMX(subst_chunk(s, VerifyArgs{phit, ppos, n_cand, np, d_qoff, q0, d_qstat, d_qwords, text, A.n, w, e, nullptr, nullptr}, sb, h_total, L));
            if (S == 2) TRY_KMX(strand_merge_chunk(s, pb.pair_stat.as<uint8_t>() + a, mb, L));
            if (rep.on()) TRY_KMX(report_chunk(s, rep, e, rb, h_total, R->found.as<uint64_t>() + Q0 + a, L));
            TRY_KMX(publish_chunk(s, who, L, Q0 + a, *R));
            a = b;
        }
        Q0 = Q1;
    }
    if (R->n_chunks == 0) R->n_chunks = 1;
    *out = R.release();
    return KMX_OK;
}

extern "C" {

kmx_status kmx_search_approx(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq, uint32_t max_subst,
                             uint32_t flags, kmx_approx_result** out)
{
    if (!index || !out) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx: NULL argument");
    return approx_search("kmx_search_approx", index, qranks, qoff, nq, max_subst, flags, nullptr, ReportOpts(), out);
}

kmx_status kmx_search_approx_strands(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq, uint32_t max_subst,
                                     uint32_t flags, const uint8_t* complement, kmx_approx_result** out)
{
    if (!index || !out) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_strands: NULL argument");
    if (!complement) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_strands: NULL complement table");
    return approx_search("kmx_search_approx_strands", index, qranks, qoff, nq, max_subst, flags, complement, ReportOpts(), out);
}

kmx_status kmx_search_approx_opts(const kmx_index* index, const uint8_t* qranks, const uint64_t* qoff, uint64_t nq,
                                  const kmx_approx_options* options, kmx_approx_result** out)
{
    if (!index || !out) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_opts: NULL argument");
    if (!options) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_opts: NULL options");
    if (options->struct_size < sizeof(kmx_approx_options))
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_opts: struct_size is smaller than kmx_approx_options");
    const uint32_t flags = options->flags;
    if (flags & ~uint32_t(KMX_APPROX_EDIT | KMX_APPROX_LOCI | KMX_APPROX_BEST))
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_opts: unknown flag bits");
    if ((flags & KMX_APPROX_LOCI) && !(flags & KMX_APPROX_EDIT))
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_search_approx_opts: KMX_APPROX_LOCI needs KMX_APPROX_EDIT");
    ReportOpts rep;
    rep.api = true;
    rep.loci = (flags & KMX_APPROX_LOCI) != 0;
    rep.best = (flags & KMX_APPROX_BEST) != 0;
    rep.max_hits = options->max_hits;
    return approx_search("kmx_search_approx_opts", index, qranks, qoff, nq, options->max_subst, flags & KMX_APPROX_EDIT, options->complement, rep, out);
}

kmx_status kmx_approx_found(kmx_approx_result* r, const uint64_t** found)
{
    if (!r) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_found: result is NULL");
    if (!r->opts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_found: the result is not one of kmx_search_approx_opts");
    if (!r->reported && r->found_lazy.size() != r->nq + 1) {     // no option was set: the list lengths
        const uint64_t* ho = r->hit_off.as<uint64_t>();
        r->found_lazy.assign(r->nq + 1, 0);
        for (uint64_t i = 0; i < r->nq; ++i) r->found_lazy[i] = ho[i + 1] - ho[i];
    }
    if (found) *found = r->reported ? r->found.as<uint64_t>() : r->found_lazy.data();
    return KMX_OK;
}

kmx_status kmx_approx_counts(const kmx_approx_result* r, uint64_t* nq, uint64_t* n_hits, uint64_t* n_candidates, uint32_t* n_chunks)
{
    if (!r) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_counts: result is NULL");
    if (nq) *nq = r->nq;
    if (n_hits) *n_hits = r->n_hits;
    if (n_candidates) *n_candidates = r->n_candidates;
    if (n_chunks) *n_chunks = r->n_chunks;
    return KMX_OK;
}

kmx_status kmx_approx_view(kmx_approx_result* r, const uint64_t** hit_off, const uint32_t** positions, const uint8_t** mismatches,
                           const uint8_t** status)
{
    if (!r) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_view: result is NULL");
    if (hit_off) *hit_off = r->hit_off.as<uint64_t>();
    if (positions) *positions = r->positions.as<uint32_t>();
    if (mismatches) *mismatches = r->mismatches.as<uint8_t>();
    if (status) *status = r->status.as<uint8_t>();
    return KMX_OK;
}

kmx_status kmx_approx_lengths(kmx_approx_result* r, const uint32_t** lengths)
{
    if (!r) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_lengths: result is NULL");
    if (!r->edit) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_lengths: the result is not one of a KMX_APPROX_EDIT call");
    if (lengths) *lengths = r->lengths.as<uint32_t>();
    return KMX_OK;
}

kmx_status kmx_approx_strands(kmx_approx_result* r, const uint8_t** strands)
{
    if (!r) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_strands: result is NULL");
    if (!r->strands) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_approx_strands: the result is not one of kmx_search_approx_strands");
    if (strands) *strands = r->strand.as<uint8_t>();
    return KMX_OK;
}

void kmx_approx_free(kmx_approx_result* r) { delete r; }

} // extern "C"
