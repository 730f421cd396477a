// Streaming 1x1 GEMM for large maps with short K (the BiFPN pointwise convs and the det-tower layers, forward and data gradient):
//   hn_conv_gemm_nt_stream : out[m][co] = act(bf16(sum_k x[m][k] w[co][k] + bias[co]))   plain pixel rows, KP <= 128, 64 < Nout <= 128
// The contract is hn_conv_gemm_nt's on that domain (hn_gemm.hip, the 64 x 64 tile of its small_tile branch), bit for bit: the same
// 16x16x32 bf16 MFMA sequence in the same K order, the same bf16 rounding points, one partial statistics row per 64-row pixel tile with
// the same in-tile summation order.  What differs is how the work is scheduled.  There, one workgroup computes one 64 x 64 tile and exits:
// for Nout = 112 every 64 pixel rows cost two fetches of the X tile and two of a weight tile, and nothing of the next tile is in flight
// while a tile is multiplied, reduced and stored.  Here a persistent workgroup
//   * loads the whole [Nout][KP] weight operand into LDS once (256-byte rows, 16-byte pieces XOR-swizzled by the row on the source side),
//   * walks 64-row pixel tiles of a static partition (no atomics, no flags, no waits on another workgroup: it cannot hang),
//   * multiplies both cout halves from ONE X tile, staged by LDS-DMA as whole 256-byte rows into a ring of NB tiles: the requests of the
//     next NB - 1 tiles are issued before a tile's MFMAs, and the steady state waits on counted vmcnt, never on vmcnt(0),
//   * stages the bf16 tile through the X slot it has just consumed to 16-byte row stores, and folds the statistics as the 64 x 64 tile does.
// 512 threads = 8 waves as 4 (32 couts) x 2 (32 pixels): the 32 x 32 wave tile of the 64 x 64 tile, its two cout workgroups side by side,
// so the statistics keep their order: per channel (q_j0 + q_j1 in a lane, DPP row sum) per pixel half, then half 0 + half 1.  (Measured:
// four waves with 64 x 32 wave tiles are 8-10 % slower, and so is giving the LDS-DMA requests and the stores to two waves each.)
// vmcnt counts a wave's stores as well as its loads, and the write-out stores of tile i - 1 are older than the requests of the newest
// tile: a wait that leaves only the LPT * (newer tiles) newest operations outstanding may wait for some of those stores too, never for
// fewer requests than it must (loads retire in order among themselves).
#include "hn_common.h"

// 16 zero bytes: the source of every out-of-range piece of an LDS-DMA (rows past M, channels past C0, weight rows past Nout)
static __device__ __attribute__((aligned(16))) bf16 g_stream_zero_piece[8];

__device__ __forceinline__ void glds16s(const bf16* src, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// 256-byte LDS rows (128 bf16): physical 16-byte piece = piece ^ (row & 15).  A ds_read_b128 whose lanes & 15 walk 16 consecutive rows at
// one logical piece touches 16 distinct slots of the 256-byte bank line; lanes >> 4 differ in the piece's low bits, which permutes the
// slots inside aligned groups of four rows, so any 16-lane group of the instruction stays conflict-free.
__device__ __forceinline__ int swz256(int row, int piece) { return row * 256 + ((piece ^ (row & 15)) << 4); }

struct GemmStream {
    const bf16* x; int ld0, C0; long M;
    const bf16* w; int Nout, KP;
    const float* bias; int act;
    bf16* out; int ldc;
    float* psum; float* psq;
    int tiles;
};

#define HN_STREAM_XT (64 * 256)      // one X tile slot: 64 rows x 256 bytes (also the staged output tile [64][128] bf16)
#define HN_STREAM_NT 512             // threads: 8 waves
#define HN_STREAM_LPT 2              // LDS-DMA instructions per thread per X tile (64 rows x 16 pieces / 512 threads)

// raw barrier: LDS writes / reads of this wave are complete (lgkmcnt), LDS-DMA of later tiles stays in flight (no vmcnt(0) as
// __syncthreads() would emit)
#define HN_STREAM_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

template <int NB>
__global__ __launch_bounds__(HN_STREAM_NT, 2) void gemm_nt_stream_kernel(const GemmStream p) {
    constexpr int TC = 2, TP = 2, WC = 32, WP = 32, BC = 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // ONE array: [WROWS][256] weights | NB X slots | wave sums [2][128][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave >> 1, wp = wave & 1;
    const int wrows = (p.Nout + 15) & ~15;
    char* sWt = smem;
    char* sX0 = smem + wrows * 256;
    float* red = reinterpret_cast<float*>(sX0 + NB * HN_STREAM_XT);

    // static partition: the workgroups are dealt to NG groups (the 8 XCDs when the grid has that many: hardware id & 7), group k owns the
    // tiles [k T / NG, (k + 1) T / NG) -- the row-order placement of xcd_remap -- and its j-th workgroup walks them with the group's stride
    const int G = gridDim.x, NG = G < 8 ? G : 8;
    const int grp = blockIdx.x % NG, j0 = blockIdx.x / NG, ngrp = (G - grp + NG - 1) / NG;
    const int t_lo = (int)((long)p.tiles * grp / NG), t_hi = (int)((long)p.tiles * (grp + 1) / NG);
    int t_cur = t_lo + j0;
    if (t_cur >= t_hi) return;                                        // no tile: nothing to load, nothing to wait for

    // LDS-DMA staging: a wave instruction writes 64 x 16 B = 4 consecutive 256-byte rows (lane-linear).  Thread t owns PHYSICAL piece
    // t & 15 of rows (t >> 4) + 32 i; the swizzle is applied on the SOURCE side: it fetches logical piece (t & 15) ^ (row & 15).
    const int r0 = tid >> 4, lp = (tid & 15) ^ (r0 & 15), ch = lp * 8;          // (row & 15 == r0 for every i)
    const bool xcv = ch < p.C0, wcv = ch < p.KP;
    auto issue_x = [&](int tile, int slot) {
        char* sX = sX0 + slot * HN_STREAM_XT;
#pragma unroll
        for (int i = 0; i < HN_STREAM_LPT; ++i) {
            const long m = (long)tile * 64 + r0 + 32 * i;
            const bf16* src = (xcv && m < p.M) ? p.x + m * p.ld0 + ch : g_stream_zero_piece;
            glds16s(src, sX + (wave * 4 + 32 * i) * 256);
        }
    };
    // bias: the couts of a workgroup are the same for every tile.  Requested first and consumed in front of the loop (below), so that no
    // wait on these registers is left inside the loop, where it would drain the tiles in flight.
    float pbias[TC][4];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
        const int co0 = wc * WC + i * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) pbias[i][r] = (p.bias && co0 + r < p.Nout) ? p.bias[co0 + r] : 0.f;
    }
    for (int i = 0; i < (wrows + 31) / 32; ++i) {                     // resident weights: rows past Nout and pieces past KP read zeros
        const int co = r0 + 32 * i;
        const bf16* src = (wcv && co < p.Nout) ? p.w + (long)co * p.KP + ch : g_stream_zero_piece;
        if (wave * 4 + 32 * i < wrows) glds16s(src, sWt + (wave * 4 + 32 * i) * 256);      // (wave-uniform: wrows is a multiple of 16)
    }
    // the first NB - 1 tiles go out back to back; t_iss = the next tile to request (requests stop at the partition's end)
    int t_iss = t_cur, n_iss = 0;                                     // n_iss: tiles requested and not yet waited for
#pragma unroll
    for (int s = 0; s < NB - 1; ++s) {
        if (t_iss < t_hi) { issue_x(t_iss, s); t_iss += ngrp; ++n_iss; }
    }
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(pbias[i][r]));      // the bias has arrived (older than every LDS-DMA request)
    const int ksteps = p.KP >> 5;
    const bool want_stats = p.psum != nullptr;
    int slot = 0, slot_iss = NB - 1;

    for (; t_cur < t_hi; t_cur += ngrp) {
        // (1) every thread has finished reading the staged tile of the previous iteration out of slot_iss: request tile t_iss into it
        HN_STREAM_BARRIER();
        if (t_iss < t_hi) { issue_x(t_iss, slot_iss); t_iss += ngrp; ++n_iss; }
        slot_iss = slot_iss + 1 == NB ? 0 : slot_iss + 1;
        // (2) tile t_cur (and the weights) have landed: at most the n_iss - 1 newer tiles' requests may be outstanding.  Loads retire in
        // order, so the count holds whatever the stores of the previous write-out (older than the newest request) do.
        if (NB >= 3 && n_iss >= 3) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * HN_STREAM_LPT) : "memory");
        else if (n_iss >= 2) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(HN_STREAM_LPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        --n_iss;

        char* sX = sX0 + slot * HN_STREAM_XT;
        f32x4 acc[TC][TP];
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps; ++ks) {
            bf16x8 a[TC], b[TP];
            const int piece = ks * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < TC; ++i)
                if (wc * WC + i * 16 < p.Nout) a[i] = *reinterpret_cast<const bf16x8*>(sWt + swz256(wc * WC + i * 16 + (lane & 15), piece));
#pragma unroll
            for (int j = 0; j < TP; ++j) b[j] = *reinterpret_cast<const bf16x8*>(sX + swz256(wp * WP + j * 16 + (lane & 15), piece));
#pragma unroll
            for (int i = 0; i < TC; ++i)
                if (wc * WC + i * 16 < p.Nout) {                      // (wave-uniform: 16-cout groups past Nout are neither read nor stored)
#pragma unroll
                    for (int j = 0; j < TP; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
                }
        }
        if (ksteps & 1) {                                             // the 64 x 64 tile walks K in stages of 64: an odd 32-chunk count ends
            const bf16x8 z = zero8();                                 // with one MFMA step over zeros (it turns a -0 sum into +0)
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TP; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(z, z, acc[i][j], 0, 0, 0);
        }

        // ---- epilogue (the staged bf16 epilogue of gemm_nt_kernel): bias, statistics of the bf16-rounded value, activation, LDS tile
        const long p_blk = (long)t_cur * 64;
        float vv[TC * TP * 4];
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) vv[(i * TP + j) * 4 + r] = acc[i][j][r] + pbias[i][r];
        // (3) every wave is done reading the X slot: it now holds the staged output tile
        HN_STREAM_BARRIER();
        if (want_stats) {
#pragma unroll
            for (int i = 0; i < TC; ++i) {
                float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < TP; ++j) {
                    const bool pv = p_blk + wp * WP + j * 16 + (lane & 15) < p.M;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float q = bfround(vv[(i * TP + j) * 4 + r]);
                        q = pv ? q : 0.f;
                        s1[r] += q;
                        s2[r] += q * q;
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s1[r] = row16_sum(s1[r]);
                    s2[r] = row16_sum(s2[r]);
                }
                if ((lane & 15) == 0) {
                    const int cl = wc * WC + i * 16 + (lane >> 4) * 4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { red[(wp * BC + cl + r) * 2] = s1[r]; red[(wp * BC + cl + r) * 2 + 1] = s2[r]; }
                }
            }
        }
        act_fwd_n(vv, p.act);
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            const int col = wc * WC + i * 16 + (lane >> 4) * 4;
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const int prow_l = wp * WP + j * 16 + (lane & 15);
                const float* v = vv + (i * TP + j) * 4;
                bf16x4 t = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                *reinterpret_cast<bf16x4*>(sX + prow_l * 256 + ((((col >> 3) ^ prow_l) & 15) << 4) + ((col >> 2) & 1) * 8) = t;
            }
        }
        // (4) tile and wave sums are written
        HN_STREAM_BARRIER();
        if (want_stats && tid < p.Nout) {                             // one partial row per pixel tile: the two pixel halves in fixed order
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int k = 0; k < 2; ++k) { t1 += red[(k * BC + tid) * 2]; t2 += red[(k * BC + tid) * 2 + 1]; }
            p.psum[(long)t_cur * p.Nout + tid] = t1;
            if (p.psq) p.psq[(long)t_cur * p.Nout + tid] = t2;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + HN_STREAM_NT * u, row = idx >> 4, pc = idx & 15;
            const long pix = p_blk + row;
            const int co = pc * 8;
            if (pix < p.M && co < p.Nout) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(sX + row * 256 + (((pc ^ row) & 15) << 4));
                *reinterpret_cast<bf16x8*>(p.out + pix * p.ldc + co) = v;
            }
        }
        slot = slot + 1 == NB ? 0 : slot + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// The domain: the small_tile branch of hn_conv_gemm_nt (knobs 4 / 5: one partial statistics row per 64 pixel rows) at 64 < Nout <= 128
// with the whole K extent in one 256-byte LDS row.
extern "C" int hn_nt_stream_ok(long M, int C0, int Nout, int KP) {
    const long max_rows = g_hn_knob[4] > g_hn_knob[5] ? g_hn_knob[4] : g_hn_knob[5];
    return M > 0 && M <= max_rows && KP > 0 && (KP & 31) == 0 && KP <= 128 && Nout > 64 && Nout <= 128 && (Nout & 7) == 0 && C0 > 0 &&
           (C0 & 7) == 0 && C0 <= KP;
}

static size_t stream_lds(int Nout, int nb) { return (size_t)((Nout + 15) & ~15) * 256 + (size_t)nb * HN_STREAM_XT + 2 * 128 * 2 * sizeof(float); }

// workgroup slots of the current device (2 per CU), cached per device id
static int stream_slots() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int v = cache[dev].load(std::memory_order_acquire);
    if (v == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
        v = 2 * cus;
        cache[dev].store(v, std::memory_order_release);
    }
    return v;
}

extern "C" int hn_conv_gemm_nt_stream(const void* x, int ld0, long M, int C0, const void* w, int Nout, int KP, const float* bias, int act,
                                      void* out, int ldc, float* psum, float* psq, int wg_limit, hipStream_t st) {
    HN_CHECK_ARG(x && w && out && wg_limit >= 0 && (!psq || psum) && ld0 >= C0 && ldc >= Nout);
    const auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!hn_nt_stream_ok(M, C0, Nout, KP) || (ld0 & 7) || (ldc & 7) || !a16(x) || !a16(w) || !a16(out)) return HN_ERR_UNSUPPORTED;
    GemmStream p;
    p.x = (const bf16*)x; p.ld0 = ld0; p.C0 = C0; p.M = M;
    p.w = (const bf16*)w; p.Nout = Nout; p.KP = KP;
    p.bias = bias; p.act = act;
    p.out = (bf16*)out; p.ldc = ldc;
    p.psum = psum; p.psq = psq;
    p.tiles = cdiv(M, 64);
    const int slots = stream_slots();
    if (slots <= 0) return HN_ERR_LAUNCH;
    // two workgroups per CU must fit the 160 KB of LDS: three X slots where the weights leave room for them (Nout <= 112), else two
    const int nb = 2 * stream_lds(Nout, 3) <= 160 * 1024 ? 3 : 2;
    const size_t lds = stream_lds(Nout, nb);
    static std::atomic<unsigned long long> optin{0};
    if (!lds_optin(optin, {(const void*)gemm_nt_stream_kernel<2>, (const void*)gemm_nt_stream_kernel<3>})) return HN_ERR_LAUNCH;
    int grid = wg_limit > 0 ? wg_limit : p.tiles;
    if (grid > slots) grid = slots;
    if (nb == 3) hipLaunchKernelGGL((gemm_nt_stream_kernel<3>), dim3(grid), dim3(HN_STREAM_NT), lds, st, p);
    else hipLaunchKernelGGL((gemm_nt_stream_kernel<2>), dim3(grid), dim3(HN_STREAM_NT), lds, st, p);
    HN_LAUNCH_CHECK();
}
