// Affine-gap local realignment of the scripts (kmx_scripts_realign; include/kmx.h, KMX_REALIGN): every entry of a scripts handle
// aligned again, locally and with affine gaps (Gotoh), inside the rectangle read x text[start, end) and the band |j - i| <= dist of
// its script, into an ordinary clips handle.  tests/realign_naive.py is the contract, cell by cell.
//
//   k_realign_prepare  a thread per entry: its read (a binary search in read_sel_off), whether the band is run for it (the script has
//                      runs, the locus and the read are inside their arrays, m > 0), the bytes of its traceback codes and its run
//                      reservation (m + L + 2); the largest entry, the entries per class
//   k_script_cut       (kmx_script_core.h) where the chunk that starts at entry e0 ends
//   k_realign_dp<NPL>  a wave per entry of the chunk, the classes and the LDS staging of k_script_dp (kmx_script.hip): the band by rows,
//                      NPL neighbouring diagonals per lane.  Per slot H and F of the previous row are kept: the diagonal predecessor
//                      is the lane's own slot, the upper one (H and F) the right neighbour's.  E along the row is a max-plus prefix
//                      scan across the lanes of Ht = max(Z, diagonal, F) with the weight x per step: opening a gap right behind one
//                      that closed never beats extending it, because o >= 0, so Ht stands for H there.  The two "opened" bits
//                      compare with the full H of the left / upper neighbour, as the contract writes them.  Per cell four bits leave
//                      through four ballots per diagonal slot (the choice of H: 0 stop, 1 diagonal, 2 E, 3 F; E opened; F opened):
//                      row i of an entry is 4 * NPL words, lane t keeps row (i - 1) % 64 and the wave stores 64 rows at a time.
//                      Every lane keeps its best (V, -i, -j) as one 64-bit key; a wave reduction leaves (i1, j1, V) of the entry.
//   k_realign_walk     a thread per entry of the chunk: the state machine of the contract from (i1, j1) along the codes; '=' and 'X'
//                      are told apart by the letters themselves.  The runs go backwards into the entry's reservation, sr S first
//                      and sl S last.  An entry that is not realigned (an empty path, V < min_score, no band) gets KMX_CLIP_LOW.
//   k_realign_whole    a thread per entry: a LOW entry gets the runs of its script, their score W[R] and their X + I + D lengths,
//                      as kmx_scripts_clip leaves a LOW entry; n_clipped and n_low through LDS and one atomic per workgroup
//   k_realign_compact  a thread per entry: its runs moved to cigar[cig_off[e] ...]
//
// -inf.  The device holds kNeg = -2^28 in a cell that does not exist, in every state.  A real H is >= -p >= -65535, and E / F of a
// cell that a path can reach are >= -65535 - o - (2d + 1) x > -4 * 10^5.  A value derived from kNeg is met one step from a cell that
// does not exist (E of the band's left edge, F of its upper edge) and stays below kNeg + 255 * 502; the cell's H is max(Z, ...) and so
// real again.  No real value reaches those, so no comparison of the traceback takes one for the other, and the walk only reads cells
// on the optimal path, whose values are real: the choice of -inf cannot change a result.  The sums stay inside int: the least is
// 2 kNeg - o - 500 x.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_clips.h"
#include "kmx_kernels.h"
#include "kmx_runs.h"
#include "kmx_script_core.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr int kNeg = -(1 << 28);
constexpr int kKeyBias = 1 << 20;                              // V + kKeyBias > 0: V >= -2 * 65535
enum { CTR_CLIPS = CTR_SHARED, CTR_COUNT = CTR_CLIPS + kmx::CL_COUNT };          // the clips' counters follow the band's

using kmx::Buf;
using kmx::grid_for;

// the scripts that are realigned
struct ScriptsIn {
    const uint64_t* read_sel_off;  // [nr + 1]
    const uint32_t* sel;           // [n_sel]
    const uint64_t* cig_off;       // [n_sel + 1]
    const uint32_t* cigar;         // [n_ops]
    uint64_t nr, n_sel, n_ops;
};

// the per-entry scratch and the chunk [e0, e1) a pass works on
struct Chunk {
    uint32_t* eread;               // the read of the entry
    uint8_t* estat;                // 1: the band is not run (no script, arrays that do not fit, the empty read)
    const uint64_t* code_off;      // bytes, multiples of 32; the arena starts at code_off[e0]
    const uint64_t* res_off;       // the run reservations
    uint64_t* arena;
    uint32_t* end_i;               // (i1, j1, V) of the entry
    uint32_t* end_j;
    int32_t* end_v;
    uint64_t e0, e1;
};

__device__ __forceinline__ uint64_t key_of(int v, uint32_t i, uint32_t j)     // greater: a greater V, then a smaller i, then a smaller j
{
    return (uint64_t(uint32_t(v + kKeyBias)) << 32) | (uint64_t(0xFFFFu - i) << 16) | uint64_t(0xFFFFu - j);
}

// ---- what the band is run for -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_realign_prepare(ScriptIn S, ScriptsIn P, Chunk C, uint32_t* __restrict__ ecode, uint32_t* __restrict__ eres,
                                                            unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t s_cls[kClasses], s_max;
    if (threadIdx.x < kClasses) s_cls[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e == 0) ctr[CTR_N_SEL] = P.n_sel;
    if (e < P.n_sel) {
        uint64_t lo = 0, hi = P.nr;                            // the read r with read_sel_off[r] <= e < read_sel_off[r + 1]; nr: none
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (P.read_sel_off[mid + 1] <= e) lo = mid + 1; else hi = mid;
        }
        uint64_t a, b;
        runs_of(P.cig_off, P.n_ops, e, &a, &b);
        const uint64_t R = b - a;
        const uint32_t l = P.sel[e];
        Entry en{};
        if (lo < P.nr && P.read_sel_off[lo] <= e && l < S.n_loci) en = entry_of(S, uint32_t(lo), l);
        const bool band = en.ok && en.m > 0 && R > 0;
        const uint32_t c = class_of(en.d);
        const uint32_t code = band ? (32u << c) * en.m : 0u;   // four words per row and diagonal slot
        C.eread[e] = lo < P.nr ? uint32_t(lo) : 0u;
        C.estat[e] = band ? 0 : 1;
        ecode[e] = code;
        eres[e] = uint32_t(max(R, uint64_t(band ? en.m + en.L + 2 : 0u)));      // the ops of a path are m + L at the most, and two S
        if (band) { atomicAdd(&s_cls[c], 1u); atomicMax(&s_max, code); }
    }
    __syncthreads();
    if (threadIdx.x < kClasses && s_cls[threadIdx.x]) atomicAdd(&ctr[CTR_CLASS + threadIdx.x], (unsigned long long)s_cls[threadIdx.x]);
    if (threadIdx.x == 0 && s_max) atomicMax(&ctr[CTR_MAX_CODE], (unsigned long long)s_max);
}

// ---- the band ------------------------------------------------------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(kWave) void k_realign_dp(ScriptIn S, ScriptsIn P, Scoring G, Chunk C)
{
    __shared__ uint8_t s_q[KMX_ALIGN_MAX_READ];
    __shared__ uint8_t s_t[kTextLds];
    const uint64_t e = C.e0 + blockIdx.x;
    if (e >= C.e1 || C.estat[e]) return;
    const uint32_t l = P.sel[e];
    if (l >= S.n_loci) return;
    const Entry en = entry_of(S, C.eread[e], l);
    if (!en.ok || en.m == 0 || (1u << class_of(en.d)) != uint32_t(NPL)) return;      // (the whole wave: one entry)
    const uint32_t lane = threadIdx.x, m = en.m, L = en.L;
    const int d = int(en.d), W = 2 * d + 1;
    stage_entry(S, en, lane, s_q, s_t);
    __syncthreads();
    uint64_t* codes = C.arena + (C.code_off[e] - C.code_off[C.e0]) / 8;
    // lane t holds the diagonals x = t * NPL + s, x = j - i + d in [0, W); cells off the band or off the text hold kNeg
    const int xb = int(lane) * NPL;
    const uint32_t lanes_used = uint32_t(W + NPL - 1) / NPL;
    const int ox = G.o + G.x;
    int ph[NPL], pf[NPL];          // H and F of the previous row
    uint32_t tl[NPL];              // the text letter t[j - 1] of the slot's cell in the row that comes
    uint64_t k0[NPL], k1[NPL], k2[NPL], k3[NPL];     // the code bits of the row this lane keeps
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
        const int j = xb + s - d;                              // row 0: H = Z(0) = 0, F does not exist
        ph[s] = xb + s < W && j >= 0 && j <= int(L) ? 0 : kNeg;
        pf[s] = kNeg;
        tl[s] = j >= 0 && j < int(L) ? s_t[j] : kNoText;       // row 1: t[j - 1] with j = 1 + x - d
        k0[s] = k1[s] = k2[s] = k3[s] = 0;
    }
    uint64_t best = key_of(-G.p, 0, 0);                        // row 0: V = -p everywhere (m > 0), the least j is 0
    for (uint32_t i = 1; i <= m; ++i) {
        uint32_t qc = s_q[i - 1];
        if (qc >= S.sigma) qc = kNoRead;
        const int z = -G.p, pen = i < m ? G.p : 0;
        int nh = __shfl_down(ph[0], 1), nf = __shfl_down(pf[0], 1);      // H and F of (i - 1, j) of the last slot: the next lane's first
        if (lane == kWave - 1) nh = nf = kNeg;
        int ht[NPL], dg[NPL], f[NPL], before[NPL];
        bool valid[NPL], fopen[NPL];
        int run = 2 * kNeg;                                    // max of Ht + x' x over the slots of this lane so far
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            const int x = xb + s, j = int(i) + x - d;
            valid[s] = x < W && j >= 0 && j <= int(L);
            const int uh = s + 1 < NPL ? ph[s + 1 < NPL ? s + 1 : s] : nh;
            const int uf = s + 1 < NPL ? pf[s + 1 < NPL ? s + 1 : s] : nf;
            const int open = uh - ox;
            f[s] = max(uf - G.x, open);
            fopen[s] = f[s] == open;
            dg[s] = ph[s] + (tl[s] == qc ? G.a : -G.b);
            ht[s] = valid[s] ? max(z, max(dg[s], f[s])) : kNeg;
            before[s] = run;
            run = max(run, ht[s] + x * G.x);
        }
        int inc = run;                                         // E = -o - x x + max over x' < x of Ht[x'] + x' x
        for (uint32_t off = 1; off < lanes_used; off <<= 1) {
            const int o = __shfl_up(inc, off);
            if (lane >= off) inc = max(inc, o);
        }
        int carry = __shfl_up(inc, 1);
        if (lane == 0) carry = 2 * kNeg;
        int h[NPL], ev[NPL];
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            const int x = xb + s;
            ev[s] = max(carry, before[s]) - G.o - x * G.x;
            h[s] = valid[s] ? max(ht[s], ev[s]) : kNeg;
            if (valid[s]) best = max(best, key_of(h[s] - pen, i, uint32_t(int(i) + x - d)));
        }
        int lh = __shfl_up(h[NPL - 1], 1);                     // the full H of (i, j - 1) of the first slot: the lane before's last
        if (lane == 0) lh = kNeg;
        const bool keeper = lane == ((i - 1) & (kWave - 1));
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            const int left = s > 0 ? h[s > 0 ? s - 1 : 0] : lh;
            // the choice of the walk: 0 stop, 1 the diagonal, 2 E, 3 F
            const uint32_t code = h[s] == z ? 0u : h[s] == dg[s] ? 1u : h[s] == ev[s] ? 2u : 3u;
            const uint64_t b0 = __ballot(code & 1u), b1 = __ballot(code >> 1);
            const uint64_t b2 = __ballot(ev[s] == left - ox), b3 = __ballot(fopen[s]);
            if (keeper) { k0[s] = b0; k1[s] = b1; k2[s] = b2; k3[s] = b3; }
            ph[s] = h[s];
            pf[s] = valid[s] ? f[s] : kNeg;
        }
#pragma unroll
        for (int s = 0; s + 1 < NPL; ++s) tl[s] = tl[s + 1];
        const int jn = int(i) + xb + NPL - 1 - d;              // row i + 1: t[j - 1] with j = i + 1 + x - d
        tl[NPL - 1] = jn >= 0 && jn < int(L) ? s_t[jn] : kNoText;
        if ((i & (kWave - 1)) == 0 || i == m) {
            const uint32_t row = ((i - 1) & ~(kWave - 1)) + lane;
            if (row < i) {
                uint64_t* p = codes + uint64_t(row) * (4 * NPL);
#pragma unroll
                for (int s = 0; s < NPL; ++s) { p[4 * s] = k0[s]; p[4 * s + 1] = k1[s]; p[4 * s + 2] = k2[s]; p[4 * s + 3] = k3[s]; }
            }
        }
    }
    for (uint32_t off = kWave / 2; off; off >>= 1) best = max(best, uint64_t(__shfl_xor((unsigned long long)best, off)));
    if (lane == 0) {
        C.end_i[e] = 0xFFFFu - uint32_t((best >> 16) & 0xFFFFu);
        C.end_j[e] = 0xFFFFu - uint32_t(best & 0xFFFFu);
        C.end_v[e] = int(uint32_t(best >> 32)) - kKeyBias;
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_realign_walk(ScriptIn S, ScriptsIn P, Scoring G, Chunk C, uint32_t* __restrict__ runs, ClipOut O)
{
    const uint64_t e = C.e0 + uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= C.e1) return;
    bool done = false;
    const uint32_t l = P.sel[e];
    if (!C.estat[e] && l < S.n_loci) {
        const Entry en = entry_of(S, C.eread[e], l);
        const uint32_t lg = class_of(en.d), W = 2 * en.d + 1;
        const uint64_t res = C.res_off[e + 1] - C.res_off[e];
        uint32_t* out = runs + C.res_off[e + 1];               // one past the reservation: the runs go in from its end
        const uint64_t* codes = C.arena + (C.code_off[e] - C.code_off[C.e0]) / 8;
        const uint32_t i1 = C.end_i[e], j1 = C.end_j[e];
        const int v = C.end_v[e];
        uint32_t i = i1, j = j1, cur = OP_NONE, len = 0, cnt = 0, nm = 0, state = 0;      // state: 0 H, 1 E, 2 F
        bool bad = !en.ok || en.m == 0 || i1 > en.m || j1 > en.L || v < G.min_score;
        if (!bad && i1 < en.m) {                               // sr S: the last run
            if (res) { out[-1] = make_run(en.m - i1, OP_S); cnt = 1; } else bad = true;
        }
        for (uint32_t step = 0; !bad; ++step) {
            if (state == 0 && i == 0) break;                   // H(0, j) = 0 = Z(0)
            const uint32_t x = j + en.d - i;                   // (wraps below 0)
            if (x >= W || i == 0 || step > 2 * (en.m + en.L) + 4) { bad = true; break; }    // (a path has m + L ops and a change of state in front of each)
            const uint64_t* p = codes + ((uint64_t(i - 1) << lg) + (x & ((1u << lg) - 1))) * 4;
            const uint32_t t = x >> lg;
            uint32_t op;
            if (state == 0) {
                const uint32_t c = uint32_t((p[0] >> t) & 1) | uint32_t(((p[1] >> t) & 1) << 1);
                if (c == 0) break;
                if (c != 1) { state = c - 1; continue; }
                if (j == 0) { bad = true; break; }
                const uint32_t qc = S.ranks[en.r0 + i - 1];
                const uint32_t tc = text_letter(S.text, S.w, uint64_t(en.start) + j - 1);
                op = qc == tc && qc < S.sigma ? OP_EQ : OP_X;
                --i;
                --j;
            } else if (state == 1) {
                if (j == 0) { bad = true; break; }
                op = OP_D;
                if ((p[2] >> t) & 1) state = 0;
                --j;
            } else {
                op = OP_I;
                if ((p[3] >> t) & 1) state = 0;
                --i;
            }
            nm += op != OP_EQ;
            if (op == cur) { ++len; continue; }
            if (len) {
                if (cnt >= res) { bad = true; break; }
                out[-1 - int64_t(cnt)] = make_run(len, cur);
                ++cnt;
            }
            cur = op;
            len = 1;
        }
        if (!bad && len) {                                     // (len == 0: an empty path)
            const uint32_t need = 1 + (i > 0 ? 1u : 0u);
            if (cnt + need > res) bad = true;
            else {
                out[-1 - int64_t(cnt)] = make_run(len, cur);
                ++cnt;
                if (i > 0) { out[-1 - int64_t(cnt)] = make_run(i, OP_S); ++cnt; }        // sl S: the first run
                O.score[e] = v;
                O.sl[e] = uint16_t(i);
                O.sr[e] = uint16_t(en.m - i1);
                O.tl[e] = uint16_t(j);
                O.tr[e] = uint16_t(en.L - j1);
                O.nm[e] = uint16_t(nm);
                O.cflags[e] = uint8_t(KMX_CLIP_REALIGNED);
                O.cnt[e] = cnt;
                done = true;
            }
        }
    }
    if (!done) O.cflags[e] = uint8_t(KMX_CLIP_LOW);            // k_realign_whole writes the rest
}

__global__ __launch_bounds__(kBlock) void k_realign_whole(ScriptsIn P, Scoring G, const uint64_t* __restrict__ res_off, uint32_t* __restrict__ runs,
                                                          ClipOut O, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[2];                          // clipped, low
    if (threadIdx.x < 2) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e < P.n_sel) {
        if (O.cflags[e] == KMX_CLIP_REALIGNED) {
            if (O.sl[e] || O.sr[e]) atomicAdd(&s_ctr[0], 1u);
        } else {
            uint64_t a, b;
            runs_of(P.cig_off, P.n_ops, e, &a, &b);
            uint64_t R = b - a;
            if (R > res_off[e + 1] - res_off[e]) R = 0;        // (never: the reservation holds the script)
            whole_entry(G, P.cigar + a, R, runs + res_off[e + 1] - R, O, e);
            atomicAdd(&s_ctr[1], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_ctr[threadIdx.x]) atomicAdd(&ctr[CTR_CLIPS + kmx::CL_N_CLIPPED + threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void k_realign_compact(uint64_t n_sel, const uint64_t* __restrict__ res_off, const uint32_t* __restrict__ runs,
                                                            const uint64_t* __restrict__ cig_off, uint64_t cap, uint32_t* __restrict__ cigar)
{
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= n_sel) return;
    const uint64_t a = cig_off[e], cnt = min(cig_off[e + 1] - a, res_off[e + 1] - res_off[e]);
    const uint32_t* from = runs + res_off[e + 1] - cnt;
    for (uint64_t k = 0; k < cnt && a + k < cap; ++k) cigar[a + k] = from[k];
}

void launch_dp(hipStream_t s, int cls, const ScriptIn& S, const ScriptsIn& P, const Scoring& G, const Chunk& C)
{
    const dim3 grid(unsigned(C.e1 - C.e0)), block(kWave);
    switch (cls) {
    case 0: hipLaunchKernelGGL(k_realign_dp<1>, grid, block, 0, s, S, P, G, C); break;
    case 1: hipLaunchKernelGGL(k_realign_dp<2>, grid, block, 0, s, S, P, G, C); break;
    case 2: hipLaunchKernelGGL(k_realign_dp<4>, grid, block, 0, s, S, P, G, C); break;
    default: hipLaunchKernelGGL(k_realign_dp<8>, grid, block, 0, s, S, P, G, C); break;
    }
}

// d_ranks / d_roff: the reads on the device of the handles; ranks_len: the letters that may be read
kmx_status realign_run(const char* fn, const kmx::IndexAccess& X, const kmx::AlignAccess& A, const kmx::ScriptsAccess& Sc, const void* d_ranks,
                       const void* d_roff, uint64_t ranks_len, const kmx_realign_options& o, hipStream_t s, kmx_clips* h)
{
    const uint64_t ns = Sc.n_sel;
    TRY_KMX(kmx::ensure_text(X, s));
    kmx_clips::Realign& x = h->re;
    TRY_HIP(x.eread.ensure(ns * 4));
    TRY_HIP(x.estat.ensure(ns));
    for (Buf* b : {&x.ecode, &x.eres}) TRY_HIP(b->ensure(ns * 4 + 16));
    for (Buf* b : {&x.code_off, &x.res_off}) TRY_HIP(b->ensure((ns + 1) * 8));
    for (Buf* b : {&x.end_i, &x.end_j, &x.end_v}) TRY_HIP(b->ensure(ns * 4));
    TRY_HIP(h->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const ScriptIn S{static_cast<const uint8_t*>(d_ranks), static_cast<const uint64_t*>(d_roff), ranks_len, nullptr, A.dist, A.start, A.end, nullptr,
                     Sc.nr, A.n_loci, X.n, X.text->d_words, X.text->w, X.sigma, 0};
    const ScriptsIn P{Sc.read_sel_off, Sc.sel, Sc.cig_off, Sc.cigar, Sc.nr, ns, Sc.n_ops};
    const Scoring G{int(o.match), int(o.mismatch), int(o.gap_open), int(o.gap_extend), int(o.clip_penalty), o.min_score};
    Chunk C{x.eread.as<uint32_t>(), x.estat.as<uint8_t>(), x.code_off.as<uint64_t>(), x.res_off.as<uint64_t>(), nullptr,
            x.end_i.as<uint32_t>(), x.end_j.as<uint32_t>(), x.end_v.as<int32_t>(), 0, 0};
    const ClipOut O{h->score.as<int32_t>(), h->sl.as<uint16_t>(), h->sr.as<uint16_t>(), h->tl.as<uint16_t>(), h->tr.as<uint16_t>(),
                    h->nm.as<uint16_t>(), h->cflags.as<uint8_t>(), h->cnt.as<uint32_t>()};
    uint64_t* bsum = h->bsum.as<uint64_t>();
    uint64_t* cig_off = h->cig_off.as<uint64_t>();
    const dim3 grid(grid_for(ns, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_realign_prepare, grid, block, 0, s, S, P, C, x.ecode.as<uint32_t>(), x.eres.as<uint32_t>(), ctr);
    kmx::launch_scan(s, x.ecode.as<uint32_t>(), ns, bsum, x.code_off.as<uint64_t>(), ctr + CTR_CODE_BYTES);
    kmx::launch_scan(s, x.eres.as<uint32_t>(), ns, bsum, x.res_off.as<uint64_t>(), ctr + CTR_RES_RUNS);
    const uint64_t want = o.scratch_bytes ? o.scratch_bytes : kDefaultScratch;
    hipLaunchKernelGGL(k_script_cut, dim3(1), dim3(1), 0, s, x.code_off.as<uint64_t>(), uint64_t(0), want, ctr);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back(fn, s, ctr, h->h_ctr, CTR_COUNT * 8));
    uint64_t c[CTR_COUNT];
    std::memcpy(c, h->h_ctr.p, sizeof c);
    const uint64_t cap = std::max(want, c[CTR_MAX_CODE]);
    TRY_HIP(ensure_exact(x.arena, std::max<uint64_t>(std::min(cap, c[CTR_CODE_BYTES]), 32)));
    TRY_HIP(x.runs.ensure(std::max<uint64_t>(c[CTR_RES_RUNS], 1) * 4));
    C.arena = x.arena.as<uint64_t>();
    C.e1 = c[CTR_CUT];
    uint32_t* runs = x.runs.as<uint32_t>();
    while (C.e0 < ns) {
        if (C.e1 <= C.e0 || C.e1 > ns) return kmx::set_error(KMX_ERR_HIP, std::string(fn) + ": an empty chunk");   // (never: the bound is clamped)
        for (int k = 0; k < kClasses; ++k)
            if (c[CTR_CLASS + k]) launch_dp(s, k, S, P, G, C);
        hipLaunchKernelGGL(k_realign_walk, dim3(grid_for(C.e1 - C.e0, kBlock)), block, 0, s, S, P, G, C, runs, O);
        C.e0 = C.e1;
        if (C.e0 < ns) {                                       // one more read-back per further chunk: where it ends
            hipLaunchKernelGGL(k_script_cut, dim3(1), dim3(1), 0, s, x.code_off.as<uint64_t>(), C.e0, want, ctr);
            TRY_HIP(hipGetLastError());
            TRY_KMX(kmx::read_back(fn, s, ctr, h->h_ctr, CTR_COUNT * 8));
            C.e1 = h->h_ctr.as<uint64_t>()[CTR_CUT];
        }
    }
    hipLaunchKernelGGL(k_realign_whole, grid, block, 0, s, P, G, x.res_off.as<uint64_t>(), runs, O, ctr);
    kmx::launch_scan(s, O.cnt, ns, bsum, cig_off, ctr + CTR_CLIPS + kmx::CL_N_OPS);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back(fn, s, ctr, h->h_ctr, CTR_COUNT * 8));      // the counts, and the runs the output holds
    std::memcpy(c, h->h_ctr.p, sizeof c);
    const uint64_t n_ops = c[CTR_CLIPS + kmx::CL_N_OPS];
    if (n_ops > c[CTR_RES_RUNS]) return kmx::set_error(KMX_ERR_HIP, std::string(fn) + ": more runs than were reserved");   // (never: a guard for the views)
    TRY_KMX(h->runs(n_ops));
    hipLaunchKernelGGL(k_realign_compact, grid, block, 0, s, ns, x.res_off.as<uint64_t>(), runs, cig_off, n_ops, h->cigar.as<uint32_t>());
    TRY_HIP(hipGetLastError());
    h->finish(ns, c + CTR_CLIPS);
    return KMX_OK;
}

// host == true: ranks / roff are host arrays that go up on the stream of the call that filled the scripts; else device arrays and
// the caller's stream
kmx_status realign_call(const char* fn, const kmx_index* index, const kmx_alignments* al, const kmx_scripts* scripts, const void* ranks,
                        const void* roff, uint64_t nr, const kmx_realign_options* o, bool host, hipStream_t stream, kmx_clips** inout)
{
    const std::string who = std::string(fn) + ": ";
    TRY_KMX(kmx::check_call(who, o, inout));
    TRY_KMX(kmx::check_scoring(who, *o));
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!al) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!scripts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "scripts handle is NULL");
    if (!roff) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "roff is NULL");
    const kmx::AlignAccess A = kmx::alignments_access(al);
    const kmx::ScriptsAccess Sc = kmx::scripts_access(scripts);
    kmx_clips* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (Sc.flags & KMX_SCRIPT_M) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts were made with KMX_SCRIPT_M: a score needs '=' and 'X' apart");
    if (nr != Sc.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "nr differs from the scripts handle's");
    if (Sc.n_sel > A.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts hold more loci than the alignments handle's n_loci");
    if (Sc.device != A.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts and the alignments live on different devices");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, Sc.device, "the scripts", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    uint64_t n_letters = ~uint64_t(0);
    if (host) {
        const char* why = kmx::check_host_reads(ranks, static_cast<const uint64_t*>(roff), nr, &n_letters);
        if (why) return refuse(KMX_ERR_INVALID_ARGUMENT, why);
    }
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, Sc.device));
    h = *inout;
    hipStream_t s = host ? Sc.stream : stream;
    kmx_status st = h->begin(s, Sc.n_sel);
    if (st == KMX_OK && Sc.n_sel) {
        const void* d_ranks = ranks;
        const void* d_roff = roff;
        if (host) {
            st = kmx::upload_reads(ranks, roff, nr, n_letters, h->re.ranks, h->re.roff, s);
            d_ranks = h->re.ranks.p;
            d_roff = h->re.roff.p;
        }
        if (st == KMX_OK) st = realign_run(fn, X, A, Sc, d_ranks, d_roff, n_letters, *o, s, h);
    }
    if (host || st != KMX_OK) (void)hipStreamSynchronize(s);   // the caller's arrays are free again; a failed call leaves nothing in flight
    if (st != KMX_OK) h->clear();                     // the handle holds an empty result, not half of this one
    return st;
}

} // namespace

extern "C" {

kmx_status kmx_scripts_realign(const kmx_index* index, const kmx_alignments* alignments, const kmx_scripts* scripts, const uint8_t* ranks,
                               const uint64_t* roff, uint64_t nr, const kmx_realign_options* options, kmx_clips** inout)
{
    return realign_call("kmx_scripts_realign", index, alignments, scripts, ranks, roff, nr, options, true, nullptr, inout);
}

kmx_status kmx_scripts_realign_device(const kmx_index* index, const kmx_alignments* alignments, const kmx_scripts* scripts, const void* d_ranks,
                                      const void* d_roff, uint64_t nr, const kmx_realign_options* options, void* stream, kmx_clips** inout)
{
    return realign_call("kmx_scripts_realign_device", index, alignments, scripts, d_ranks, d_roff, nr, options, false, static_cast<hipStream_t>(stream),
                        inout);
}

} // extern "C"
