// The pileup of the read-mapping chain (kmx_clips_pileup_device, kmx_clips_rescues_pileup, kmx_pileup_sites; include/kmx.h, KMX_PILEUP):
// the runs of every entry of a scripts or clips handle replayed against the reads into sigma + 3 planes of u32 counters over a text
// region, channel-major (counts[c * len + pos - lo]), and the positions of that region where something other than the reference
// letter is frequent.
//
//   k_pileup_check     a thread per entry: rules 1 - 3 of kmx.h (no runs, FILTERED, MISMATCHED) in one pass over the runs in front of any
//                      add: the test of k_md_count (kmx_tags.hip) extended by the read side.  Writes the verdict, the read and the text
//                      interval cut to the region; the three verdict counters through LDS and one atomic each per workgroup
//   k_pileup_add       ATOMIC path, a wave per ADDED entry: the wave walks the runs (uniform), the 64 lanes stride over the letters of a
//                      run, so consecutive lanes add to consecutive positions of a plane: no-return atomicAdd on u32, a few contiguous
//                      segments per wave-instruction.  n_cells through a wave reduction, LDS and one atomic per workgroup
//   k_sites_count      a thread per position: depth, and the candidates that pass (integer arithmetic); n_covered as above
//   k_sites_write      the same walk behind kmx::launch_scan: one record per passing (pos, channel), in that order
// Everything is integer: the result does not depend on the order in which the adds arrive.  A TILED path (the region cut into tiles, a
// workgroup per tile counting in LDS and adding its planes with plain stores) was built, measured at the probe's shapes and taken out:
// it lost to the atomic path at every one of them.  KMX_PILEUP_TILED and options.tile are still accepted and
// checked; both run this path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_kernels.h"
#include "kmx_runs.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kWaves = kBlock / kWave;
constexpr uint32_t kMinTile = 64;                              // options.tile: 0 or a power of two from here on
enum { V_NONE = 0, V_FILTERED, V_MISMATCHED, V_ADDED };
enum { PU_N_ADDED = 0, PU_N_FILTERED, PU_N_MISMATCHED, PU_N_CELLS, PU_COUNT };
enum { SI_N_SITES = 0, SI_N_COVERED, SI_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// what the pileup kernels read: the runs (of the scripts or of the clips), the start / end arrays that sel indexes, the reads
struct PileIn {
    const uint32_t* sel;           // [n_sel]
    const uint64_t* cig_off;       // [n_sel + 1]
    const uint32_t* cigar;         // [n_ops]
    const uint32_t* start;         // [bound]
    const uint32_t* end;
    const uint64_t* read_sel_off;  // [nr + 1]
    const uint8_t* ranks;          // the letters of the reads, at most ranks_len
    const uint64_t* roff;          // [nr + 1]
    const uint16_t* tl;            // [n_sel]: the clips' values; all nullptr for the scripts' own runs
    const uint16_t* tr;
    const int32_t* score;
    const uint8_t* cflags;
    const uint8_t* mapq;           // [nr / 2], or nullptr
    uint64_t n_sel, n_ops, bound, nr, ranks_len, n, lo, hi;
    uint32_t sigma, flags, min_mapq;
    int32_t min_score;
};

// the per-entry values k_pileup_check leaves for the kernels behind it
struct Verdicts {
    uint8_t* verdict;              // [n_sel]: V_*
    uint32_t* read;                // the read of an ADDED entry
    uint64_t* c0;                  // [c0, c1): its text interval [t0, t1) cut to the region (empty: nothing to add)
    uint64_t* c1;
};

__global__ __launch_bounds__(kBlock) void k_pileup_check(PileIn P, Verdicts E, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[3];                          // added, filtered, mismatched
    if (threadIdx.x < 3) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e < P.n_sel) {
        uint64_t a, b;
        runs_of(P.cig_off, P.n_ops, e, &a, &b);
        uint32_t verdict = V_NONE, read = 0;
        uint64_t c0 = 0, c1 = 0;
        if (b > a) {                                           // (rule 1: an entry without runs moves no counter)
            uint64_t r = 0, hi = P.nr;                         // the read r with read_sel_off[r] <= e < read_sel_off[r + 1]; nr: none
            while (r < hi) {
                const uint64_t mid = (r + hi) >> 1;
                if (P.read_sel_off[mid + 1] <= e) r = mid + 1; else hi = mid;
            }
            const bool has_read = r < P.nr && P.read_sel_off[r] <= e;
            const bool clips = P.tl != nullptr;
            const bool filtered = (clips && (P.flags & KMX_PILEUP_SKIP_LOW) && (P.cflags[e] & KMX_CLIP_LOW)) || (clips && P.score[e] < P.min_score) ||
                                  (P.mapq && has_read && P.mapq[r >> 1] < P.min_mapq);
            if (filtered) verdict = V_FILTERED;
            else {
                const uint32_t l = P.sel[e];
                bool bad = l >= P.bound || !has_read;
                uint64_t m = 0, want = 0, t0 = 0, t1 = 0;
                if (!bad) {
                    const uint64_t q0 = P.roff[r], q1 = P.roff[r + 1];
                    bad = !(q0 <= q1 && q1 <= P.ranks_len);    // (a read outside the letters: no such read)
                    m = q1 - q0;
                }
                if (!bad) {
                    const uint64_t s = P.start[l], t = P.end[l];
                    bad = !(s <= t && t <= P.n);
                    want = t - s;
                    const uint64_t cl = clips ? P.tl[e] : 0, cr = clips ? P.tr[e] : 0;
                    bad = bad || cl + cr > want;
                    want -= cl + cr;
                    t0 = s + cl;
                    t1 = t - cr;
                }
                uint64_t text = 0, letters = 0;
                for (uint64_t k = a; k < b && !bad; ++k) {
                    const uint32_t v = P.cigar[k], op = run_op(v);
                    const uint64_t len = run_len(v);
                    if (op == OP_EQ || op == OP_X) { text += len; letters += len; }
                    else if (op == OP_D) text += len;
                    else if (op == OP_I) letters += len;
                    else if (op == OP_S && (k == a || k + 1 == b)) letters += len;
                    else bad = true;
                }
                bad = bad || text != want || letters != m;
                verdict = bad ? V_MISMATCHED : V_ADDED;
                if (!bad) {
                    read = uint32_t(r);
                    c0 = max(t0, P.lo);
                    c1 = max(min(t1, P.hi), c0);
                }
            }
            atomicAdd(&s_ctr[verdict == V_ADDED ? 0 : verdict == V_FILTERED ? 1 : 2], 1u);
        }
        E.verdict[e] = uint8_t(verdict);
        E.read[e] = read;
        E.c0[e] = c0;
        E.c1[e] = c1;
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_ctr[threadIdx.x]) atomicAdd(&ctr[PU_N_ADDED + threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

// The wave's walk over the runs of the ADDED entry e of read r: one atomic add for every cell with w0 <= pos < w1 ([w0, w1) lies inside
// the region), the lanes striding over the letters of a run.  Returns the cells this lane added.  k_pileup_check has found the lengths
// of the runs equal to the read's and to the interval's, so no letter past either is touched.
__device__ __forceinline__ uint32_t replay(const PileIn& P, uint64_t e, uint32_t r, uint32_t lane, uint64_t w0, uint64_t w1, uint32_t* __restrict__ counts)
{
    const uint64_t lo = P.lo, plane = P.hi - P.lo;
    auto add = [&](uint32_t c, uint64_t pos) { atomicAdd(&counts[uint64_t(c) * plane + (pos - lo)], 1u); };
    uint64_t a, b;
    runs_of(P.cig_off, P.n_ops, e, &a, &b);
    const uint32_t l = P.sel[e];
    if (l >= P.bound || r >= P.nr) return 0;                   // (cannot happen: k_pileup_check saw the same arrays)
    const uint64_t q0 = P.roff[r], m = P.roff[r + 1] - q0;
    const uint8_t* __restrict__ q = P.ranks + q0;
    const uint64_t t0 = uint64_t(P.start[l]) + (P.tl ? P.tl[e] : 0), t1 = uint64_t(P.end[l]) - (P.tr ? P.tr[e] : 0);
    uint64_t i = 0, j = t0;
    uint32_t cells = 0;
    for (uint64_t k = a; k < b && j <= w1; ++k) {              // (behind the window nothing is added any more; an I at w1 counts at w1 - 1)
        const uint32_t v = P.cigar[k], op = run_op(v);
        const uint64_t len = run_len(v);
        if (op == OP_S) i += len;
        else if (op == OP_I) {
            if (t0 < j && j < t1 && j - 1 >= w0 && j - 1 < w1 && lane == 0) { add(P.sigma + 2, j - 1); ++cells; }
            i += len;
        } else {                                               // = X D: the letters [x0, x1) of the run lie inside the window
            const uint64_t x0 = max(w0, j) - j, x1 = min(min(w1, t1), j + len) > j ? min(min(w1, t1), j + len) - j : 0;
            if (op == OP_D) {
                for (uint64_t x = x0 + lane; x < x1; x += kWave) { add(P.sigma + 1, j + x); ++cells; }
            } else {
                const uint64_t x2 = min(x1, m > i ? m - i : 0);
                for (uint64_t x = x0 + lane; x < x2; x += kWave) {
                    const uint32_t c = q[i + x];
                    add(c < P.sigma ? c : P.sigma, j + x);
                    ++cells;
                }
                i += len;
            }
            j += len;
        }
    }
    return cells;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
    return v;                                                  // (lane 0 holds the sum)
}

__global__ __launch_bounds__(kBlock) void k_pileup_add(PileIn P, Verdicts E, uint32_t* __restrict__ counts, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_cells;
    if (threadIdx.x == 0) s_cells = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t e = uint64_t(blockIdx.x) * kWaves + threadIdx.x / kWave;
    if (e < P.n_sel && E.verdict[e] == V_ADDED && E.c1[e] > E.c0[e]) {
        const uint32_t cells = wave_sum(replay(P, e, E.read[e], lane, E.c0[e], E.c1[e], counts));
        if (lane == 0 && cells) atomicAdd(&s_cells, cells);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cells) atomicAdd(&ctr[PU_N_CELLS], (unsigned long long)s_cells);
}

// ---- the sites -----------------------------------------------------------------------------------------------------------------------
struct SitesIn {
    const uint32_t* counts;        // [n_channels * len]
    const uint64_t* text;          // packed at w bits per letter
    const uint64_t* ctg_off;       // [nc + 1], or nullptr
    uint64_t lo, len, nc;
    uint32_t w, sigma, min_depth, min_alt, frac_num, frac_den;
};

struct SitesOut {
    uint32_t* pos;                 // [n_sites]
    uint8_t* ref;
    uint8_t* alt;
    uint32_t* depth;
    uint32_t* count;
    uint32_t* ref_count;
    uint32_t* ctg;                 // or nullptr
};

__device__ __forceinline__ uint32_t sat_u32(uint64_t v) { return uint32_t(min(v, uint64_t(0xFFFFFFFFull))); }

// the candidates of position x of the region, in ascending channel order: emit(channel, count) for every one that passes; returns
// false when the position is not covered
template <typename Emit>
__device__ __forceinline__ bool site_walk(const SitesIn& Q, uint64_t x, uint32_t* ref, uint64_t* depth, Emit emit)
{
    uint64_t d = 0;
    for (uint32_t c = 0; c < Q.sigma + 2; ++c) d += Q.counts[uint64_t(c) * Q.len + x];
    *depth = d;
    if (d < max(Q.min_depth, 1u)) return false;
    const uint32_t r = text_letter(Q.text, Q.w, Q.lo + x);
    *ref = r;
    for (uint32_t c = 0; c < Q.sigma + 3; ++c) {
        if (c == r || c == Q.sigma) continue;
        const uint32_t cnt = Q.counts[uint64_t(c) * Q.len + x];
        if (cnt >= max(Q.min_alt, 1u) && (unsigned __int128)cnt * Q.frac_den >= (unsigned __int128)Q.frac_num * d) emit(c, cnt);
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void k_sites_count(SitesIn Q, uint32_t* __restrict__ cnt, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_covered;
    if (threadIdx.x == 0) s_covered = 0;
    __syncthreads();
    const uint64_t x = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (x < Q.len) {
        uint32_t ref = 0, n = 0;
        uint64_t depth = 0;
        if (site_walk(Q, x, &ref, &depth, [&](uint32_t, uint32_t) { ++n; })) atomicAdd(&s_covered, 1u);
        cnt[x] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_covered) atomicAdd(&ctr[SI_N_COVERED], (unsigned long long)s_covered);
}

__global__ __launch_bounds__(kBlock) void k_sites_write(SitesIn Q, const uint64_t* __restrict__ off, uint64_t n_sites, SitesOut O)
{
    const uint64_t x = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (x >= Q.len) return;
    uint64_t at = off[x];
    const uint64_t lim = min(off[x + 1], n_sites);
    if (lim <= at) return;
    const uint64_t pos = Q.lo + x;
    uint32_t ctg = 0;
    if (O.ctg) {                                               // the contig c with ctg_off[c] <= pos < ctg_off[c + 1] (k_locate's search)
        uint64_t a = 0, b = Q.nc;
        while (a + 1 < b) {
            const uint64_t mid = (a + b) >> 1;
            if (Q.ctg_off[mid] <= pos) a = mid; else b = mid;
        }
        ctg = uint32_t(a);
    }
    uint32_t ref = 0;
    uint64_t depth = 0;
    const uint32_t* plane = Q.counts + x;
    site_walk(Q, x, &ref, &depth, [&](uint32_t c, uint32_t cnt) {
        if (at >= lim) return;
        O.pos[at] = uint32_t(pos);
        O.ref[at] = uint8_t(ref);
        O.alt[at] = uint8_t(c);
        O.depth[at] = sat_u32(depth);
        O.count[at] = cnt;
        O.ref_count[at] = ref < Q.sigma ? plane[uint64_t(ref) * Q.len] : 0u;
        if (O.ctg) O.ctg[at] = ctg;
        ++at;
    });
}

} // namespace

struct kmx_pileup {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the last call (the views and the counts synchronise on it)
    uint64_t lo = 0, hi = 0;
    uint32_t n_channels = 0, sigma = 0;    // n_channels == 0: the handle holds nothing
    kmx::ArrOf<uint32_t> counts;           // the result: cells() counters, kept across a KMX_PILEUP_ADD call and its refusals
    // the counters (read back on demand: kmx_pileup_counts), and the scratch of a call: the verdicts
    Buf ctr, verdict, read, c0, c1;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&counts}; }
    std::vector<Buf*> scratch() { return {&ctr, &verdict, &read, &c0, &c1}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { lo = hi = 0; n_channels = sigma = 0; kmx::clear_arrays(*this); }
    uint64_t cells() const { return uint64_t(n_channels) * (hi - lo); }
};

struct kmx_sites {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t n_sites = 0, n_covered = 0;
    bool with_ctg = false;
    // results: one entry per record; ctg only when the index has a contig table
    kmx::ArrOf<uint32_t> pos, depth, count, ref_count, ctg;
    kmx::ArrOf<uint8_t> ref, alt;
    Buf cnt, off, bsum, ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&pos, &ref, &alt, &depth, &count, &ref_count, &ctg}; }
    std::vector<Buf*> scratch() { return {&cnt, &off, &bsum, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { n_sites = n_covered = 0; with_ctg = false; kmx::clear_arrays(*this); }
};

namespace {

// the reads a call runs over, on the device of the scripts
struct ReadsIn {
    const void* ranks;
    const void* roff;
    uint64_t nr, ranks_len;        // ranks_len: the letters that may be read
};

kmx_status pileup_run(const PileIn& P, hipStream_t s, kmx_pileup* h)
{
    const uint64_t ns = P.n_sel;
    if (ns == 0) return KMX_OK;
    for (Buf* b : {&h->c0, &h->c1}) TRY_HIP(b->ensure(ns * 8));
    TRY_HIP(h->read.ensure(ns * 4));
    TRY_HIP(h->verdict.ensure(ns));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    uint32_t* counts = h->counts.as<uint32_t>();
    const Verdicts E{h->verdict.as<uint8_t>(), h->read.as<uint32_t>(), h->c0.as<uint64_t>(), h->c1.as<uint64_t>()};
    const dim3 grid(grid_for(ns, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_pileup_check, grid, block, 0, s, P, E, ctr);
    hipLaunchKernelGGL(k_pileup_add, dim3(grid_for(ns, kWaves)), block, 0, s, P, E, counts, ctr);      // (whatever the mode: see the head of this file)
    TRY_HIP(hipGetLastError());
    return KMX_OK;
}

// the refusals that need no handle
kmx_status pileup_front(const std::string& who, const kmx_index* index, const void* source, const char* source_name, const void* scripts,
                        const kmx_pileup_options* o, kmx_pileup** inout)
{
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags & ~uint32_t(KMX_PILEUP_ADD | KMX_PILEUP_SKIP_LOW)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "unknown flag bits");
    if (o->mode > KMX_PILEUP_TILED) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "mode > KMX_PILEUP_TILED");
    if (o->tile && (o->tile < kMinTile || (o->tile & (o->tile - 1)))) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "tile is neither 0 nor a power of two >= 64");
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!source) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + source_name + " handle is NULL");
    if (!scripts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "scripts handle is NULL");
    return KMX_OK;
}

// the pileup of the scripts S (K: their clips, whose runs and values then stand in for the scripts' own) over the start / end arrays
// (of `bound` entries, on `device`) that their sel indexes and the reads R, into *inout
kmx_status pileup_on_arrays(const char* fn, const kmx_index* index, const kmx::ScriptsAccess& S, const kmx::ClipsAccess* K, int device,
                            const uint32_t* start, const uint32_t* end, uint64_t bound, const ReadsIn& R, int reads_device, const uint8_t* d_mapq,
                            const kmx_pileup_options& o, hipStream_t stream, kmx_pileup** inout)
{
    const std::string who = std::string(fn) + ": ";
    const bool add = o.flags & KMX_PILEUP_ADD;
    kmx_pileup* h = *inout;
    auto refuse = [&](kmx_status st, const std::string& msg) {  // a handle that is added to keeps what it holds
        if (h && !add) h->clear();
        return kmx::set_error(st, who + msg);
    };
    if (S.flags & KMX_SCRIPT_M) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts were made with KMX_SCRIPT_M: a pileup needs '=' and 'X' apart");
    if (K && K->n_sel != S.n_sel) return refuse(KMX_ERR_INVALID_ARGUMENT, "the clips are not those of these scripts: n_sel differs");
    if (R.nr != S.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "nr differs from the scripts handle's");
    if (d_mapq && (R.nr & 1)) return refuse(KMX_ERR_INVALID_ARGUMENT, "a MAPQ array with an odd nr: it holds one value per pair of internal reads");
    if (S.n_sel && (S.device != device || S.device != reads_device)) return refuse(KMX_ERR_INVALID_ARGUMENT, "the handles live on different devices");
    if (K && K->n_sel && K->device != S.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the clips and the scripts live on different devices");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, S.device, "the scripts", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    const uint64_t lo = o.lo, hi = o.hi ? o.hi : X.n;
    if (lo >= hi || hi > X.n) return refuse(KMX_ERR_INVALID_ARGUMENT, "the region is empty or ends behind the text");
    const uint32_t n_channels = X.sigma + 3;
    const bool keep = add && h && h->n_channels;               // the call adds to what the handle holds
    if (keep && (h->lo != lo || h->hi != hi || h->sigma != X.sigma))
        return refuse(KMX_ERR_INVALID_ARGUMENT, "KMX_PILEUP_ADD: the region or the alphabet differs from the handle's");
    if (keep && h->device != S.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "KMX_PILEUP_ADD: the pileup lives on another device");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, S.device));
    h = *inout;
    hipStream_t s = stream ? stream : S.stream;
    h->stream = s;
    h->host_valid = false;
    (void)hipGetLastError();
    auto run = [&]() -> kmx_status {
        if (!keep) {                                           // the planes of this region, zeroed, and the counters with them
            h->clear();
            const uint64_t bytes = uint64_t(n_channels) * (hi - lo) * 4;
            TRY_HIP(h->counts.ensure(bytes));
            TRY_HIP(h->ctr.ensure(PU_COUNT * 8));
            TRY_HIP(hipMemsetAsync(h->counts.p, 0, bytes, s));
            TRY_HIP(hipMemsetAsync(h->ctr.p, 0, PU_COUNT * 8, s));
            h->lo = lo;
            h->hi = hi;
            h->sigma = X.sigma;
            h->n_channels = n_channels;
            h->counts.n = h->cells();
        }
        const PileIn P{S.sel, K ? K->cig_off : S.cig_off, K ? K->cigar : S.cigar, start, end, S.read_sel_off, static_cast<const uint8_t*>(R.ranks),
                       static_cast<const uint64_t*>(R.roff), K ? K->tl : nullptr, K ? K->tr : nullptr, K ? K->score : nullptr, K ? K->cflags : nullptr,
                       d_mapq, S.n_sel, K ? K->n_ops : S.n_ops, bound, R.nr, R.ranks_len, X.n, lo, hi, X.sigma, o.flags, o.min_mapq, o.min_score};
        return pileup_run(P, s, h);
    };
    const kmx_status st = run();
    if (st != KMX_OK) {                                        // nothing is left in flight; planes that may hold a part of this call are dropped
        (void)hipStreamSynchronize(s);
        h->clear();
    }
    return st;
}

kmx_status sites_run(const kmx::IndexAccess& X, const kmx_pileup* p, const kmx_sites_options& o, hipStream_t s, kmx_sites* h)
{
    TRY_KMX(kmx::ensure_text(X, s));
    const uint64_t len = p->hi - p->lo;
    TRY_HIP(h->cnt.ensure(len * 4 + 16));
    TRY_HIP(h->off.ensure((len + 1) * 8));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(len) * 8 + 16));
    TRY_HIP(h->ctr.ensure(SI_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, SI_COUNT * 8, s));
    const bool with_ctg = X.ctg_off && X.nc;
    const SitesIn Q{p->counts.as<uint32_t>(), X.text->d_words, with_ctg ? X.ctg_off : nullptr, p->lo, len, X.nc, X.text->w, X.sigma,
                    o.min_depth, o.min_alt, o.frac_num, o.frac_den};
    const dim3 grid(grid_for(len, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_sites_count, grid, block, 0, s, Q, h->cnt.as<uint32_t>(), ctr);
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), len, h->bsum.as<uint64_t>(), h->off.as<uint64_t>(), ctr + SI_N_SITES);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_pileup_sites", s, ctr, h->h_ctr, SI_COUNT * 8));   // the one read-back: the records size the arrays
    const uint64_t n_sites = h->h_ctr.as<uint64_t>()[SI_N_SITES];
    if (n_sites) {
        for (Buf* b : {&h->pos, &h->depth, &h->count, &h->ref_count}) TRY_HIP(b->ensure(n_sites * 4));
        for (Buf* b : {&h->ref, &h->alt}) TRY_HIP(b->ensure(n_sites));
        if (with_ctg) TRY_HIP(h->ctg.ensure(n_sites * 4));
        const SitesOut O{h->pos.as<uint32_t>(), h->ref.as<uint8_t>(), h->alt.as<uint8_t>(), h->depth.as<uint32_t>(), h->count.as<uint32_t>(),
                         h->ref_count.as<uint32_t>(), with_ctg ? h->ctg.as<uint32_t>() : nullptr};
        hipLaunchKernelGGL(k_sites_write, grid, block, 0, s, Q, h->off.as<uint64_t>(), n_sites, O);
        TRY_HIP(hipGetLastError());
    }
    h->n_sites = n_sites;
    kmx::expose(h->results(), n_sites);
    if (!with_ctg) h->ctg.n = 0;
    h->n_covered = h->h_ctr.as<uint64_t>()[SI_N_COVERED];
    h->with_ctg = with_ctg;
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_clips_pileup_device(const kmx_index* index, const kmx_alignments* alignments, const kmx_scripts* scripts, const kmx_clips* clips,
                                   const void* d_ranks, const void* d_roff, uint64_t nr, const uint8_t* d_mapq, const kmx_pileup_options* options,
                                   void* stream, kmx_pileup** inout)
{
    const std::string who = "kmx_clips_pileup_device: ";
    TRY_KMX(pileup_front(who, index, alignments, "alignments", scripts, options, inout));
    if (!d_roff) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "d_roff is NULL");
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    const kmx::ScriptsAccess S = kmx::scripts_access(scripts);
    kmx::ClipsAccess K{};
    if (clips) K = kmx::clips_access(clips);
    const ReadsIn R{d_ranks, d_roff, nr, ~uint64_t(0)};
    return pileup_on_arrays("kmx_clips_pileup_device", index, S, clips ? &K : nullptr, A.device, A.start, A.end, A.n_loci, R, S.device, d_mapq, *options,
                            static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_clips_rescues_pileup(const kmx_index* index, const kmx_strand_reads* reads, const kmx_rescues* rescues, const kmx_scripts* scripts,
                                    const kmx_clips* clips, const uint8_t* d_mapq, const kmx_pileup_options* options, void* stream,
                                    kmx_pileup** inout)
{
    const std::string who = "kmx_clips_rescues_pileup: ";
    TRY_KMX(pileup_front(who, index, rescues, "rescues", scripts, options, inout));
    if (!reads) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "reads handle is NULL");
    const kmx::JobsAccess J = kmx::rescues_access(rescues);
    const kmx::ScriptsAccess S = kmx::scripts_access(scripts);
    kmx::ClipsAccess K{};
    if (clips) K = kmx::clips_access(clips);
    const ReadsIn R{reads->ranks2.p, reads->roff2.p, reads->nr2, reads->letters2};
    return pileup_on_arrays("kmx_clips_rescues_pileup", index, S, clips ? &K : nullptr, J.device, J.start, J.end, J.n_jobs, R, reads->device, d_mapq,
                            *options, static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_pileup_counts(kmx_pileup* p, uint64_t* lo, uint64_t* hi, uint32_t* n_channels, uint64_t* n_added, uint64_t* n_filtered,
                             uint64_t* n_mismatched, uint64_t* n_cells)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_pileup_counts: pileup handle is NULL");
    uint64_t c[PU_COUNT] = {};
    if (p->n_channels) {                                       // the counters of the kernels in flight: wait for them
        kmx::DeviceGuard dg;
        TRY_HIP(hipSetDevice(p->device));
        TRY_KMX(kmx::read_back("kmx_pileup_counts", p->stream, p->ctr.p, p->h_ctr, PU_COUNT * 8));
        std::memcpy(c, p->h_ctr.p, sizeof c);
    }
    if (lo) *lo = p->lo;
    if (hi) *hi = p->hi;
    if (n_channels) *n_channels = p->n_channels;
    if (n_added) *n_added = c[PU_N_ADDED];
    if (n_filtered) *n_filtered = c[PU_N_FILTERED];
    if (n_mismatched) *n_mismatched = c[PU_N_MISMATCHED];
    if (n_cells) *n_cells = c[PU_N_CELLS];
    return KMX_OK;
}

kmx_status kmx_pileup_view_device(const kmx_pileup* p, const uint32_t** d_counts)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_pileup_view_device: pileup handle is NULL");
    if (d_counts) *d_counts = p->counts.dev();
    return KMX_OK;
}

kmx_status kmx_pileup_view(kmx_pileup* p, const uint32_t** counts)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_pileup_view: pileup handle is NULL");
    if (p->n_channels == 0) {                                  // the empty handle: no array
        if (counts) *counts = nullptr;
        return KMX_OK;
    }
    TRY_KMX(kmx::host_view("kmx_pileup_view", *p));            // 4 bytes per channel and position
    if (counts) *counts = p->counts.host();
    return KMX_OK;
}

void kmx_pileup_free(kmx_pileup* p) { kmx::free_handle(p); }

kmx_status kmx_pileup_sites(const kmx_index* index, const kmx_pileup* pileup, const kmx_sites_options* o, void* stream, kmx_sites** inout)
{
    const std::string who = "kmx_pileup_sites: ";
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->frac_den == 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "frac_den is 0");
    if (o->frac_num > o->frac_den) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "frac_num > frac_den");
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!pileup) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "pileup handle is NULL");
    kmx_sites* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (pileup->n_channels == 0) return refuse(KMX_ERR_INVALID_ARGUMENT, "the pileup holds nothing");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, pileup->device, "the pileup", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    if (pileup->n_channels != X.sigma + 3 || pileup->hi > X.n) return refuse(KMX_ERR_INVALID_ARGUMENT, "the pileup is not one over this index: its channels or its region do not fit");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, pileup->device));
    h = *inout;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : pileup->stream;
    return kmx::run_into(h, s, [&] { return sites_run(X, pileup, *o, s, h); });
}

kmx_status kmx_sites_counts(const kmx_sites* h, uint64_t* n_sites, uint64_t* n_covered)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_sites_counts: sites handle is NULL");
    if (n_sites) *n_sites = h->n_sites;
    if (n_covered) *n_covered = h->n_covered;
    return KMX_OK;
}

kmx_status kmx_sites_view_device(const kmx_sites* h, const uint32_t** d_pos, const uint8_t** d_ref, const uint8_t** d_alt, const uint32_t** d_depth,
                                 const uint32_t** d_count, const uint32_t** d_ref_count, const uint32_t** d_ctg)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_sites_view_device: sites handle is NULL");
    if (d_pos) *d_pos = h->pos.dev();
    if (d_ref) *d_ref = h->ref.dev();
    if (d_alt) *d_alt = h->alt.dev();
    if (d_depth) *d_depth = h->depth.dev();
    if (d_count) *d_count = h->count.dev();
    if (d_ref_count) *d_ref_count = h->ref_count.dev();
    if (d_ctg) *d_ctg = h->ctg.dev();
    return KMX_OK;
}

kmx_status kmx_sites_view(kmx_sites* h, const uint32_t** pos, const uint8_t** ref, const uint8_t** alt, const uint32_t** depth,
                          const uint32_t** count, const uint32_t** ref_count, const uint32_t** ctg)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_sites_view: sites handle is NULL");
    TRY_KMX(kmx::host_view("kmx_sites_view", *h));             // 18 bytes per record, 22 with ctg
    if (pos) *pos = h->pos.host();
    if (ref) *ref = h->ref.host();
    if (alt) *alt = h->alt.host();
    if (depth) *depth = h->depth.host();
    if (count) *count = h->count.host();
    if (ref_count) *ref_count = h->ref_count.host();
    if (ctg) *ctg = h->with_ctg ? h->ctg.host() : nullptr;
    return KMX_OK;
}

void kmx_sites_free(kmx_sites* h) { kmx::free_handle(h); }

} // extern "C"
