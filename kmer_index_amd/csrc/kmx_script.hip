// Edit scripts of the alignments (kmx_alignments_scripts, include/kmx.h): for every selected locus the one canonical script of the
// global alignment of the read and text[start, end), as BAM-style runs.  The ends and the distance d are known, so the DP is
// confined to the 2d + 1 diagonals |j - i| <= d.
//
//   k_script_count     a thread per read: how many of its loci are selected (the best one, or every aligned one)
//   k_script_select    a thread per read: sel[], the read of every entry and, per entry, whether it can be served, the bytes of its
//                      traceback codes and its run reservation (2d + 1); the totals, the largest entry, the entries per class
//   k_script_cut       one thread: where the chunk that starts at entry e0 ends (the last entry whose codes still fit the arena);
//                      it lives in kmx_script_core.h, with the entry's bounds and the LDS staging, which kmx_realign.hip shares
//   k_script_dp<NPL>   a wave per entry of the chunk: the band by rows, NPL neighbouring diagonals per lane (NPL in {1, 2, 4, 8}, the
//                      smallest with 64 * NPL >= 2d + 1; a wave of another class leaves at once).  The diagonal predecessor is the
//                      lane's own value of the previous row, the upper one its right neighbour's, the chain along the row a min-plus
//                      prefix scan across the lanes.  Per cell the choice of the walk (2 bits) leaves through two ballots per
//                      diagonal slot: row i of an entry is 2 * NPL words, lane t keeps row (i - 1) % 64 and the wave stores 64 rows
//                      at a time.  Nothing else of H is kept.  H[m][L] != d marks the entry as mismatched.
//   k_script_walk      a thread per entry of the chunk: from (m, L) to (0, 0) along the codes, runs written backwards into the
//                      entry's reservation, the run count left behind
//   k_script_compact   a thread per entry: its runs moved to cigar[cig_off[e] ...]
// Read and text letters of an entry are staged in LDS (the text from the packed copy, one 64-bit word per lane at a time:
// stage_entry, kmx_script_core.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_kernels.h"
#include "kmx_runs.h"
#include "kmx_script_core.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr int kInf = 1 << 20;                                 // beyond any distance; sums of a few of them stay inside int
constexpr uint32_t kNoBest = 0xFFFFFFFFu;
enum { CTR_N_OPS = CTR_SHARED, CTR_N_MISMATCHED, CTR_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// the per-entry arrays and the chunk [e0, e1) a pass works on
struct Entries {
    const uint32_t* sel;           // locus of the entry
    const uint32_t* eread;         // its read
    uint8_t* estat;                // 1: mismatched (no script)
    const uint64_t* code_off;      // bytes, multiples of 16; the arena starts at code_off[e0]
    uint64_t* arena;
    unsigned long long* ctr;
    uint64_t e0, e1;
};

// the loci of read r that are selected, in ascending order: f(l) for each
template <typename F>
__device__ __forceinline__ void for_selected(const ScriptIn& S, uint64_t r, F f)
{
    const uint64_t a = S.locus_off[r], b = min(S.locus_off[r + 1], S.n_loci);
    if (S.flags & KMX_SCRIPT_ALL) {
        for (uint64_t l = a; l < b; ++l)
            if (S.dist[l] < KMX_ALIGN_SKIPPED) f(uint32_t(l));
    } else {
        const uint32_t bi = S.best[r];
        if (bi != kNoBest && a + bi < b) f(uint32_t(a + bi));
    }
}

// ---- selection -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_script_count(ScriptIn S, uint32_t* __restrict__ cnt)
{
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= S.nr) return;
    uint32_t c = 0;
    for_selected(S, r, [&](uint32_t) { ++c; });
    cnt[r] = c;
}

__global__ __launch_bounds__(kBlock) void k_script_select(ScriptIn S, const uint64_t* __restrict__ read_sel_off, uint64_t cap_e,
                                                          uint32_t* __restrict__ sel, uint32_t* __restrict__ eread, uint8_t* __restrict__ estat,
                                                          uint32_t* __restrict__ ecode, uint32_t* __restrict__ eres, unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t s_cls[kClasses], s_bad, s_max;
    if (threadIdx.x < kClasses) s_cls[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_bad = 0; s_max = 0; }
    __syncthreads();
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r < S.nr) {
        uint64_t e = read_sel_off[r];
        for_selected(S, r, [&](uint32_t l) {
            if (e >= cap_e) return;                            // (cannot happen: the scan counted these very loci)
            const Entry en = entry_of(S, uint32_t(r), l);
            const uint32_t c = class_of(en.d);
            const uint32_t code = en.ok ? (16u << c) * en.m : 0u;   // two words per row and diagonal slot
            sel[e] = l;
            eread[e] = uint32_t(r);
            estat[e] = en.ok ? 0 : 1;
            ecode[e] = code;
            eres[e] = en.ok ? 2 * en.d + 1 : 0u;
            if (!en.ok) atomicAdd(&s_bad, 1u);
            else if (en.m) { atomicAdd(&s_cls[c], 1u); atomicMax(&s_max, code); }
            ++e;
        });
    }
    __syncthreads();
    if (threadIdx.x < kClasses && s_cls[threadIdx.x]) atomicAdd(&ctr[CTR_CLASS + threadIdx.x], (unsigned long long)s_cls[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (s_bad) atomicAdd(&ctr[CTR_N_MISMATCHED], (unsigned long long)s_bad);
        if (s_max) atomicMax(&ctr[CTR_MAX_CODE], (unsigned long long)s_max);
    }
}

// ---- the band ------------------------------------------------------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(kWave) void k_script_dp(ScriptIn S, Entries C)
{
    __shared__ uint8_t s_q[KMX_ALIGN_MAX_READ];
    __shared__ uint8_t s_t[kTextLds];
    const uint64_t e = C.e0 + blockIdx.x;
    if (e >= C.e1 || C.estat[e]) return;
    const Entry en = entry_of(S, C.eread[e], C.sel[e]);
    if (!en.ok || en.m == 0 || (1u << class_of(en.d)) != uint32_t(NPL)) return;      // (the whole wave: one entry)
    const uint32_t lane = threadIdx.x, m = en.m, L = en.L;
    const int d = int(en.d), W = 2 * d + 1;
    stage_entry(S, en, lane, s_q, s_t);
    __syncthreads();
    uint64_t* codes = C.arena + (C.code_off[e] - C.code_off[C.e0]) / 8;
    // lane t holds the diagonals x = t * NPL + s, x = j - i + d in [0, W); cells off the band or off the text hold kInf
    const int xb = int(lane) * NPL;
    const uint32_t lanes_used = uint32_t(W + NPL - 1) / NPL;
    int prev[NPL];
    uint32_t tl[NPL];              // the text letter t[j - 1] of the slot's cell in the row that comes
    uint64_t k0[NPL], k1[NPL];     // the code bits of the row this lane keeps
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
        const int j = xb + s - d;                              // row 0: H[0][j] = j
        prev[s] = xb + s < W && j >= 0 && j <= int(L) ? j : kInf;
        tl[s] = j >= 0 && j < int(L) ? s_t[j] : kNoText;       // row 1: t[j - 1] with j = 1 + x - d
        k0[s] = k1[s] = 0;
    }
    for (uint32_t i = 1; i <= m; ++i) {
        uint32_t qc = s_q[i - 1];
        if (qc >= S.sigma) qc = kNoRead;
        int nb = __shfl_down(prev[0], 1);                      // H[i - 1][j] of the last slot: the next lane's first
        if (lane == kWave - 1) nb = kInf;
        int u[NPL], dg[NPL], before[NPL];
        bool valid[NPL];
        int run = kInf;                                        // min of u - x over the slots of this lane so far
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            const int x = xb + s, j = int(i) + x - d;
            valid[s] = x < W && j >= 0 && j <= int(L);
            const int up = (s + 1 < NPL ? prev[s + 1 < NPL ? s + 1 : s] : nb) + 1;
            dg[s] = prev[s] + int(tl[s] != qc);
            u[s] = valid[s] ? min(dg[s], up) : kInf;
            before[s] = run;
            run = min(run, u[s] - x);
        }
        int inc = run;                                         // the chain along the row: H = min over x' <= x of u[x'] + (x - x')
        for (uint32_t off = 1; off < lanes_used; off <<= 1) {
            const int o = __shfl_up(inc, off);
            if (lane >= off) inc = min(inc, o);
        }
        int carry = __shfl_up(inc, 1);
        if (lane == 0) carry = kInf;
        const bool keeper = lane == ((i - 1) & (kWave - 1));
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            const int x = xb + s;
            const int left = min(carry, before[s]) + x;        // H[i][j - 1] + 1
            const int h = valid[s] ? min(min(u[s], left), kInf) : kInf;
            // the choice of the walk: 0 '=', 1 'X', 2 'D', 3 'I'
            const uint32_t code = dg[s] == h ? uint32_t(tl[s] != qc) : left == h ? 2u : 3u;
            const uint64_t b0 = __ballot(code & 1u), b1 = __ballot(code >> 1);
            if (keeper) { k0[s] = b0; k1[s] = b1; }
            prev[s] = h;
        }
#pragma unroll
        for (int s = 0; s + 1 < NPL; ++s) tl[s] = tl[s + 1];
        const int jn = int(i) + xb + NPL - 1 - d;              // row i + 1: t[j - 1] with j = i + 1 + x - d
        tl[NPL - 1] = jn >= 0 && jn < int(L) ? s_t[jn] : kNoText;
        if ((i & (kWave - 1)) == 0 || i == m) {
            const uint32_t row = ((i - 1) & ~(kWave - 1)) + lane;
            if (row < i) {
                uint64_t* p = codes + uint64_t(row) * (2 * NPL);
#pragma unroll
                for (int s = 0; s < NPL; ++s) { p[2 * s] = k0[s]; p[2 * s + 1] = k1[s]; }
            }
        }
    }
    const int xs = int(L) - int(m) + d;                        // (m, L): in [0, W) because |m - L| <= d
#pragma unroll
    for (int s = 0; s < NPL; ++s)
        if (xb + s == xs && prev[s] != d) {                    // one lane: not the reads of this alignment
            C.estat[e] = 1;
            atomicAdd(&C.ctr[CTR_N_MISMATCHED], 1ull);
        }
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_script_walk(ScriptIn S, Entries C, const uint64_t* __restrict__ run_off, uint32_t* __restrict__ runs,
                                                        uint32_t* __restrict__ eruns)
{
    const uint64_t e = C.e0 + uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= C.e1) return;
    uint32_t cnt = 0;
    if (!C.estat[e]) {
        const Entry en = entry_of(S, C.eread[e], C.sel[e]);
        const uint32_t lg = class_of(en.d), W = 2 * en.d + 1;
        const uint64_t res = run_off[e + 1] - run_off[e];      // 2d + 1
        uint32_t* out = runs + run_off[e + 1];                 // one past the reservation: the runs go in from its end
        const uint64_t* codes = C.arena + (C.code_off[e] - C.code_off[C.e0]) / 8;
        const bool as_m = (S.flags & KMX_SCRIPT_M) != 0;
        uint32_t i = en.m, j = en.L, cur = OP_NONE, len = 0;
        bool bad = !en.ok;
        while (!bad && (i | j)) {
            uint32_t op;
            if (i == 0) op = OP_D;
            else if (j == 0) op = OP_I;
            else {
                const uint32_t x = j + en.d - i;               // (wraps below 0)
                if (x >= W) { bad = true; break; }
                const uint64_t* p = codes + ((uint64_t(i - 1) << lg) + (x & ((1u << lg) - 1))) * 2;
                const uint32_t t = x >> lg;
                const uint32_t c = uint32_t((p[0] >> t) & 1) | uint32_t(((p[1] >> t) & 1) << 1);
                op = c == 0 ? OP_EQ : c == 1 ? OP_X : c == 2 ? OP_D : OP_I;
            }
            if (op != OP_D) --i;
            if (op != OP_I) --j;
            if (as_m && op >= OP_EQ) op = OP_M;
            if (op == cur) { ++len; continue; }
            if (len) {
                if (cnt >= res) { bad = true; break; }
                out[-1 - int64_t(cnt)] = make_run(len, cur);
                ++cnt;
            }
            cur = op;
            len = 1;
        }
        if (!bad && len) {
            if (cnt >= res) bad = true;
            else { out[-1 - int64_t(cnt)] = make_run(len, cur); ++cnt; }
        }
        if (bad) {                                             // (only with foreign reads, and then the band has caught it already)
            cnt = 0;
            C.estat[e] = 1;
            atomicAdd(&C.ctr[CTR_N_MISMATCHED], 1ull);
        }
    }
    eruns[e] = cnt;
}

__global__ __launch_bounds__(kBlock) void k_script_compact(const unsigned long long* __restrict__ ctr, const uint64_t* __restrict__ run_off,
                                                           const uint32_t* __restrict__ runs, const uint64_t* __restrict__ cig_off,
                                                           uint32_t* __restrict__ cigar)
{
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= ctr[CTR_N_SEL]) return;
    const uint64_t a = cig_off[e], cnt = cig_off[e + 1] - a;
    const uint32_t* from = runs + run_off[e + 1] - cnt;
    for (uint64_t k = 0; k < cnt; ++k) cigar[a + k] = from[k];
}

} // namespace

struct kmx_scripts {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_sel = 0, n_ops = 0, n_mismatched = 0;
    uint32_t flags = 0;                    // the options' flags of the call that filled the handle (kmx_scripts_md refuses KMX_SCRIPT_M)
    // results
    kmx::ArrOf<uint64_t> read_sel_off{kmx::ARR_OFFSETS}, cig_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<uint32_t> sel, cigar;
    // scratch
    Buf ranks, roff, cnt, bsum, eread, estat, ecode, eres, eruns, code_off, run_off, arena, runs, ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&read_sel_off, &sel, &cig_off, &cigar}; }
    std::vector<Buf*> scratch() { return {&ranks, &roff, &cnt, &bsum, &eread, &estat, &ecode, &eres, &eruns, &code_off, &run_off, &arena, &runs, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_sel = n_ops = n_mismatched = 0; kmx::clear_arrays(*this); }
    // a call has succeeded: the arrays expose what the counters say
    void expose()
    {
        read_sel_off.n = nr + 1;
        sel.n = n_sel;
        cig_off.n = n_sel + 1;
        cigar.n = n_ops;
    }
};

namespace {

void launch_dp(hipStream_t s, int cls, const ScriptIn& S, const Entries& C)
{
    const dim3 grid(unsigned(C.e1 - C.e0)), block(kWave);
    switch (cls) {
    case 0: hipLaunchKernelGGL(k_script_dp<1>, grid, block, 0, s, S, C); break;
    case 1: hipLaunchKernelGGL(k_script_dp<2>, grid, block, 0, s, S, C); break;
    case 2: hipLaunchKernelGGL(k_script_dp<4>, grid, block, 0, s, S, C); break;
    default: hipLaunchKernelGGL(k_script_dp<8>, grid, block, 0, s, S, C); break;
    }
}

// d_ranks / d_roff: the reads on the device of the handles; ranks_len: the letters that may be read; best: what selects the
// entries, the alignments' own or a caller's in its place (kmx_placements_scripts)
kmx_status script_run(const kmx::IndexAccess& X, const kmx::LociAccess& L, const kmx::AlignAccess& A, const void* d_ranks, const void* d_roff,
                      uint64_t ranks_len, const uint32_t* best, const kmx_script_options& o, hipStream_t s, kmx_scripts* h)
{
    const uint64_t nr = L.nr, nl = L.n_loci;
    h->flags = o.flags;
    TRY_HIP(h->read_sel_off.ensure((nr + 1) * 8));
    if (nr == 0 || nl == 0) {                                  // no entry: no launch indexes an empty array
        TRY_HIP(h->cig_off.ensure(8));
        TRY_HIP(hipMemsetAsync(h->read_sel_off.p, 0, (nr + 1) * 8, s));
        TRY_HIP(hipMemsetAsync(h->cig_off.p, 0, 8, s));
        h->nr = nr;
        h->expose();
        return KMX_OK;
    }
    TRY_KMX(kmx::ensure_text(X, s));
    const bool all = (o.flags & KMX_SCRIPT_ALL) != 0;
    const uint64_t cap_e = all ? nl : std::min(nr, nl);       // entries at the most (nl < 2^32: kmx_loci_align)
    TRY_HIP(h->cnt.ensure(nr * 4 + 16));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(std::max(nr, cap_e)) * 8 + 16));
    TRY_HIP(h->sel.ensure(cap_e * 4));
    TRY_HIP(h->eread.ensure(cap_e * 4));
    TRY_HIP(h->estat.ensure(cap_e));
    for (Buf* b : {&h->ecode, &h->eres, &h->eruns}) TRY_HIP(b->ensure(cap_e * 4 + 16));
    for (Buf* b : std::initializer_list<Buf*>{&h->code_off, &h->run_off, &h->cig_off}) TRY_HIP(b->ensure((cap_e + 1) * 8));
    TRY_HIP(h->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    for (Buf* b : {&h->ecode, &h->eres, &h->eruns}) TRY_HIP(hipMemsetAsync(b->p, 0, cap_e * 4, s));   // the scans run over cap_e entries
    const ScriptIn S{static_cast<const uint8_t*>(d_ranks), static_cast<const uint64_t*>(d_roff), ranks_len, L.locus_off, A.dist, A.start, A.end, best,
                     nr, nl, X.n, X.text->d_words, X.text->w, X.sigma, o.flags};
    uint64_t* bsum = h->bsum.as<uint64_t>();
    hipLaunchKernelGGL(k_script_count, dim3(grid_for(nr, kBlock)), dim3(kBlock), 0, s, S, h->cnt.as<uint32_t>());
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), nr, bsum, h->read_sel_off.as<uint64_t>(), ctr + CTR_N_SEL);
    hipLaunchKernelGGL(k_script_select, dim3(grid_for(nr, kBlock)), dim3(kBlock), 0, s, S, h->read_sel_off.as<uint64_t>(), cap_e, h->sel.as<uint32_t>(),
                       h->eread.as<uint32_t>(), h->estat.as<uint8_t>(), h->ecode.as<uint32_t>(), h->eres.as<uint32_t>(), ctr);
    kmx::launch_scan(s, h->ecode.as<uint32_t>(), cap_e, bsum, h->code_off.as<uint64_t>(), ctr + CTR_CODE_BYTES);
    kmx::launch_scan(s, h->eres.as<uint32_t>(), cap_e, bsum, h->run_off.as<uint64_t>(), ctr + CTR_RES_RUNS);
    const uint64_t want = o.scratch_bytes ? o.scratch_bytes : kDefaultScratch;
    hipLaunchKernelGGL(k_script_cut, dim3(1), dim3(1), 0, s, h->code_off.as<uint64_t>(), uint64_t(0), want, ctr);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_alignments_scripts", s, ctr, h->h_ctr, CTR_COUNT * 8));
    uint64_t c[CTR_COUNT];
    std::memcpy(c, h->h_ctr.p, sizeof c);
    const uint64_t n_sel = c[CTR_N_SEL];
    if (n_sel > cap_e) return kmx::set_error(KMX_ERR_HIP, "kmx_alignments_scripts: more entries than loci");      // (never: a guard for the arrays)
    if (n_sel) {
        const uint64_t cap = std::max(want, c[CTR_MAX_CODE]);
        TRY_HIP(ensure_exact(h->arena, std::max<uint64_t>(std::min(cap, c[CTR_CODE_BYTES]), 16)));
        TRY_HIP(h->runs.ensure(std::max<uint64_t>(c[CTR_RES_RUNS], 1) * 4));
        TRY_HIP(h->cigar.ensure(std::max<uint64_t>(c[CTR_RES_RUNS], 1) * 4));  // a script fills its reservation at the most
        Entries C{h->sel.as<uint32_t>(), h->eread.as<uint32_t>(), h->estat.as<uint8_t>(), h->code_off.as<uint64_t>(), h->arena.as<uint64_t>(), ctr, 0, c[CTR_CUT]};
        while (C.e0 < n_sel) {
            if (C.e1 <= C.e0 || C.e1 > n_sel) return kmx::set_error(KMX_ERR_HIP, "kmx_alignments_scripts: an empty chunk");  // (never: the bound is clamped)
            for (int k = 0; k < kClasses; ++k)
                if (c[CTR_CLASS + k]) launch_dp(s, k, S, C);
            hipLaunchKernelGGL(k_script_walk, dim3(grid_for(C.e1 - C.e0, kBlock)), dim3(kBlock), 0, s, S, C, h->run_off.as<uint64_t>(), h->runs.as<uint32_t>(),
                               h->eruns.as<uint32_t>());
            C.e0 = C.e1;
            if (C.e0 < n_sel) {                                // one more read-back per further chunk: where it ends
                hipLaunchKernelGGL(k_script_cut, dim3(1), dim3(1), 0, s, h->code_off.as<uint64_t>(), C.e0, want, ctr);
                TRY_HIP(hipGetLastError());
                TRY_KMX(kmx::read_back("kmx_alignments_scripts", s, ctr, h->h_ctr, CTR_COUNT * 8));
                C.e1 = h->h_ctr.as<uint64_t>()[CTR_CUT];
            }
        }
    }
    kmx::launch_scan(s, h->eruns.as<uint32_t>(), cap_e, bsum, h->cig_off.as<uint64_t>(), ctr + CTR_N_OPS);
    if (n_sel)
        hipLaunchKernelGGL(k_script_compact, dim3(grid_for(n_sel, kBlock)), dim3(kBlock), 0, s, ctr, h->run_off.as<uint64_t>(), h->runs.as<uint32_t>(),
                           h->cig_off.as<uint64_t>(), h->cigar.as<uint32_t>());
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_alignments_scripts", s, ctr, h->h_ctr, CTR_COUNT * 8));
    h->nr = nr;
    h->n_sel = n_sel;
    h->n_ops = h->h_ctr.as<uint64_t>()[CTR_N_OPS];
    h->n_mismatched = h->h_ctr.as<uint64_t>()[CTR_N_MISMATCHED];
    h->expose();
    return KMX_OK;
}

kmx_status check_front(const char* fn, const kmx_index* index, const kmx_loci* loci, const kmx_alignments* al, const void* roff,
                       const kmx_script_options* o, kmx_scripts** inout)
{
    const std::string who = std::string(fn) + ": ";
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!al) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!o) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options is NULL");
    if (!inout) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout is NULL");
    if (!roff) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "roff is NULL");
    if (o->struct_size < sizeof(kmx_script_options)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options->struct_size is too small");
    if (o->flags & ~(KMX_SCRIPT_ALL | KMX_SCRIPT_M)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "unknown flags");
    return KMX_OK;
}

// host == true: ranks / roff are host arrays that go up on the stream of the call that filled the alignments; else device arrays
// and the caller's stream.  P != nullptr: its best2 selects in the place of the alignments' best (device form; ranks_len letters may
// be read)
kmx_status script_call(const char* fn, const kmx_index* index, const kmx_loci* loci, const kmx_alignments* al, const void* ranks, const void* roff,
                       uint64_t nr, const kmx_script_options* o, bool host, hipStream_t stream, kmx_scripts** inout,
                       const kmx::PlacementsAccess* P = nullptr, uint64_t ranks_len = ~uint64_t(0))
{
    TRY_KMX(check_front(fn, index, loci, al, roff, o, inout));
    const std::string who = std::string(fn) + ": ";
    if (P && (o->flags & KMX_SCRIPT_ALL)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "KMX_SCRIPT_ALL ignores best: not for the winners of a fold");
    const kmx::LociAccess L = kmx::loci_access(loci);
    const kmx::AlignAccess A = kmx::alignments_access(al);
    kmx_scripts* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (nr != L.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "nr differs from the loci handle's");
    if (nr != A.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "nr differs from the alignments handle's");
    if (A.n_loci != L.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's n_loci differs from the loci handle's");
    if (A.device != L.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the loci and the alignments live on different devices");
    if (P && P->nr2 != nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements are not those of these reads: nr differs");
    if (P && nr && P->device != L.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements and the loci live on different devices");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, L.device, "the loci", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    uint64_t n_letters = ranks_len;
    if (host) {
        const char* why = kmx::check_host_reads(ranks, static_cast<const uint64_t*>(roff), nr, &n_letters);
        if (why) return refuse(KMX_ERR_INVALID_ARGUMENT, why);
    }
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, L.device));
    h = *inout;
    hipStream_t s = host ? A.stream : stream;
    const kmx_status st = kmx::run_into(h, s, [&] {
        const void* d_ranks = ranks;
        const void* d_roff = roff;
        if (host && nr && L.n_loci) {
            TRY_KMX(kmx::upload_reads(ranks, roff, nr, n_letters, h->ranks, h->roff, s));
            d_ranks = h->ranks.p;
            d_roff = h->roff.p;
        }
        return script_run(X, L, A, d_ranks, d_roff, n_letters, P ? P->best2 : A.best, *o, s, h);
    });
    if (host && st == KMX_OK) (void)hipStreamSynchronize(s);   // the caller's arrays are free again
    return st;
}

} // namespace

kmx::ScriptsAccess kmx::scripts_access(const kmx_scripts* s)
{
    return ScriptsAccess{s->device, s->stream, s->n_sel, s->n_ops, s->flags, s->sel.as<uint32_t>(), s->cig_off.as<uint64_t>(), s->cigar.as<uint32_t>(),
                         s->nr, s->read_sel_off.as<uint64_t>()};
}

kmx_status kmx::scripts_with_best(const char* fn, const kmx_index* index, const kmx_loci* loci, const kmx_alignments* alignments, const void* d_ranks,
                                  const void* d_roff, uint64_t nr, uint64_t ranks_len, const kmx_script_options* options, hipStream_t stream,
                                  const kmx::PlacementsAccess& P, kmx_scripts** inout)
{
    return script_call(fn, index, loci, alignments, d_ranks, d_roff, nr, options, false, stream, inout, &P, ranks_len);
}

kmx_status kmx::scripts_on_arrays(const char* fn, const kmx_index* index, const kmx::LociAccess& L, const kmx::AlignAccess& A, const void* d_ranks,
                                  const void* d_roff, uint64_t ranks_len, const uint32_t* best, const kmx_script_options* o, hipStream_t stream,
                                  kmx_scripts** inout, bool every)
{
    const std::string who = std::string(fn) + ": ";
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags & ~(KMX_SCRIPT_ALL | KMX_SCRIPT_M)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "unknown flags");
    if (o->flags & KMX_SCRIPT_ALL)
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + (every ? "KMX_SCRIPT_ALL is not the caller's to set: every entry has a script already"
                                                                     : "KMX_SCRIPT_ALL ignores best: not for the taken jobs of a rescue"));
    kmx_script_options run = *o;                               // (struct_size may be larger: only the known fields are read)
    run.struct_size = sizeof run;
    if (every) run.flags |= KMX_SCRIPT_ALL;
    kmx_scripts* h = *inout;
    auto refuse = kmx::refuser(who, h);
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, L.device, "the arrays", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, L.device));
    h = *inout;
    return kmx::run_into(h, stream, [&] { return script_run(X, L, A, d_ranks, d_roff, ranks_len, best, run, stream, h); });
}

extern "C" {

kmx_status kmx_alignments_scripts(const kmx_index* index, const kmx_loci* loci, const kmx_alignments* alignments, const uint8_t* ranks,
                                  const uint64_t* roff, uint64_t nr, const kmx_script_options* options, kmx_scripts** inout)
{
    return script_call("kmx_alignments_scripts", index, loci, alignments, ranks, roff, nr, options, true, nullptr, inout);
}

kmx_status kmx_alignments_scripts_device(const kmx_index* index, const kmx_loci* loci, const kmx_alignments* alignments, const void* d_ranks,
                                         const void* d_roff, uint64_t nr, const kmx_script_options* options, void* stream, kmx_scripts** inout)
{
    return script_call("kmx_alignments_scripts_device", index, loci, alignments, d_ranks, d_roff, nr, options, false, static_cast<hipStream_t>(stream),
                       inout);
}

kmx_status kmx_scripts_counts(const kmx_scripts* h, uint64_t* nr, uint64_t* n_sel, uint64_t* n_ops, uint64_t* n_mismatched)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_scripts_counts: scripts handle is NULL");
    if (nr) *nr = h->nr;
    if (n_sel) *n_sel = h->n_sel;
    if (n_ops) *n_ops = h->n_ops;
    if (n_mismatched) *n_mismatched = h->n_mismatched;
    return KMX_OK;
}

kmx_status kmx_scripts_view_device(const kmx_scripts* h, const uint64_t** d_read_sel_off, const uint32_t** d_sel, const uint64_t** d_cig_off,
                                   const uint32_t** d_cigar)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_scripts_view_device: scripts handle is NULL");
    if (d_read_sel_off) *d_read_sel_off = h->read_sel_off.dev();
    if (d_sel) *d_sel = h->sel.dev();
    if (d_cig_off) *d_cig_off = h->cig_off.dev();
    if (d_cigar) *d_cigar = h->cigar.dev();
    return KMX_OK;
}

kmx_status kmx_scripts_view(kmx_scripts* h, const uint64_t** read_sel_off, const uint32_t** sel, const uint64_t** cig_off, const uint32_t** cigar)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_scripts_view: scripts handle is NULL");
    TRY_KMX(kmx::host_view("kmx_scripts_view", *h));
    if (read_sel_off) *read_sel_off = h->read_sel_off.host();
    if (sel) *sel = h->sel.host();
    if (cig_off) *cig_off = h->cig_off.host();
    if (cigar) *cigar = h->cigar.host();
    return KMX_OK;
}

void kmx_scripts_free(kmx_scripts* h) { kmx::free_handle(h); }

} // extern "C"
