// PNG label encode on the device (png_encode.py; semantics in DESIGN.md 4l, restated in numpy by tests/png_enc_ref.py): class maps (int64
// [N, Hs, Ws] masks or packed uint8 maps) -> per image a complete zlib stream of the filtered scanlines of the map resized to (Ho, Wo):
// what goes into a PNG file's IDAT chunk.  One memset of N words and four launches over a ragged batch (grid.y = image), each reading what
// the previous one left in the workspace; no workgroup waits on another.
//   pngenc_filter_kernel         one workgroup per output row: cv2's INTER_NEAREST index rule (aug_seg_kernel's), the five PNG filters on
//                                the resized pixels (bpp = 1), the smallest sum of |(int8) byte| picks the filter (ties: the lowest number);
//                                the filter byte and the filtered row go to the image's raw region.  Rows are independent: an encoding
//                                filter reads unfiltered pixels, which every row gathers from the source itself.  An int64 value outside
//                                0..255 that the resize samples raises the image's range flag (a plain store of 1 into a zeroed word).
//   pngenc_deflate_kernel<false> one workgroup per chunk of PNGENC_CHUNK raw bytes: its bit count as one fixed-Huffman block, and the
//                                chunk's Adler-32 partial sums.
//   pngenc_scan_kernel           one workgroup per image: 64-bit exclusive bit offsets of the chunks behind the two header bytes, the
//                                Adler-32 fold, the status and the result record; it zeroes the words two chunks share (and the trailer's),
//                                then ORs the header 78 01 and the big-endian Adler-32 into them.
//   pngenc_deflate_kernel<true>  the same parse again, now with the chunk's bit offset: every token is ORed into the chunk's span in LDS,
//                                whole words go out with plain stores, the span's first and last word with atomicOr into the zeroed words
//                                (order-independent: deterministic bytes).
// How the token chain is found: every thread owns 16 consecutive positions of the chunk.  It builds two 16-bit equality masks
// (raw[p] == raw[p - 1], raw[p] == raw[p - S]); the run of equal bytes that starts at a position is the run inside the owner's mask plus,
// when the mask is all ones from there, a carry gathered from the following masks (at most 17 of them: lengths stop at 258).  That gives the
// greedy step of EVERY position at once (the longer of the two matches when >= 3, ties to distance 1, else a literal) in an LDS table; one
// lane then walks the table from the chunk's first byte and flags the token starts -- at most PNGENC_CHUNK trips, a handful for the
// near-constant rows a label map filters to.  Bit counts of the flagged tokens, a block prefix sum, and every thread emits its own.
// Every loop is bounded by the chunk size, every store by the image's raw size / capacity; no address depends on pixel data other than
// through the token bit counts, which the capacity check bounds before anything is stored.  All integer (the resize index in float64, with
// FMA contraction off, as the numpy restatement writes it), exact.
// hn_png_encode_dyn (second half of the file; restated by tests/png_enc_dyn_ref.py) shares the filter, the parse and the scan and writes one
// block per 16 chunks with a Huffman code built from the block's own tokens where that is smaller than the fixed code.
#include "hn_common.h"

#pragma clang fp contract(off)

#define PNGENC_ST_RANGE 1              // an int64 value outside 0..255
#define PNGENC_ST_FULL 2               // the stream is longer than the image's capacity
#define PNGENC_ST_RECORD 3             // the record does not fit the buffers

#define PNGENC_CHUNK 4096              // raw bytes per deflate block (= 16 per thread)
#define PNGENC_THREADS 256
#define PNGENC_MAX_LEN 258
#define PNGENC_WINDOW 32768
#define PNGENC_SPAN_WORDS ((31 + 9 * PNGENC_CHUNK + 10 + 31) / 32 + 1)
#define PNGENC_ADLER_MOD 65521u
static_assert(PNGENC_CHUNK == 16 * PNGENC_THREADS && PNGENC_CHUNK >= 512 && PNGENC_CHUNK <= 32768, "16 positions per thread");

namespace {

struct PngEncDesc {                    // png_encode.py DESC_DTYPE (64 bytes)
    long src_off;                      // the map's first element in src (elements: int64 or bytes)
    long raw_off;                      // its filtered scanlines inside ws (a multiple of 16)
    long out_off;                      // its stream inside out (a multiple of 4)
    long out_cap;                      // bytes the stream may use there (a multiple of 4)
    int Hs, Ws, Ho, Wo;
    long pad[2];
};
static_assert(sizeof(PngEncDesc) == 64, "PngEncDesc layout is mirrored by png_encode.py");

struct PngEncResult {                  // png_encode.py RESULT_DTYPE (16 bytes)
    long stream_bytes;                 // 0 unless status == 0
    int status, pad;
};

struct PngEncLayout {                  // ws: the raw regions, one range flag per image, then per chunk its bits, bit offset and Adler sums
    long raw_region, flag_off, bits_off, off_off, part_off, nchunk, total;
};

__host__ __device__ inline PngEncLayout pngenc_layout(long n, long max_raw) {
    PngEncLayout l;
    l.raw_region = n * ((max_raw + 15) & ~15L);
    l.nchunk = (max_raw + PNGENC_CHUNK - 1) / PNGENC_CHUNK;
    l.flag_off = l.raw_region;
    l.bits_off = l.flag_off + ((n * 4 + 15) & ~15L);
    l.off_off = l.bits_off + ((n * l.nchunk * 4 + 15) & ~15L);
    l.part_off = l.off_off + n * l.nchunk * 8;
    l.total = l.part_off + n * l.nchunk * 8;
    return l;
}

__device__ __forceinline__ long pngenc_raw_bytes(const PngEncDesc& d) { return (long)d.Ho * (1 + (long)d.Wo); }

// the record's extents against the buffers handed to the entry point (uniform per image)
__device__ __forceinline__ bool pngenc_fits(const PngEncDesc& d, long src_elems, int max_h, long max_raw, long raw_region, long out_bytes) {
    if (!(d.Hs >= 1 && d.Hs <= 65535 && d.Ws >= 1 && d.Ws <= 65535 && d.Ho >= 1 && d.Ho <= 65535 && d.Wo >= 1 && d.Wo <= 65535)) return false;
    const long raw = pngenc_raw_bytes(d);
    return d.Ho <= max_h && raw <= max_raw && d.src_off >= 0 && d.src_off + (long)d.Hs * d.Ws <= src_elems && d.raw_off >= 0 &&
           (d.raw_off & 15) == 0 && d.raw_off + ((raw + 15) & ~15L) <= raw_region && d.out_off >= 0 && (d.out_off & 3) == 0 &&
           d.out_cap >= 0 && (d.out_cap & 3) == 0 && d.out_off + d.out_cap <= out_bytes;
}

// exclusive prefix sum over the PNGENC_THREADS threads of a workgroup; *total: the sum.  sh: 4 words of LDS, free to reuse after the call.
__device__ __forceinline__ unsigned long long pngenc_block_scan(unsigned long long v, unsigned long long* sh, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                                     // the previous call's reads of sh
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < PNGENC_THREADS / 64; ++w) {
        const unsigned long long t = sh[w];
        if (w < wave) base += t;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------------ resize + row filter

struct PngEncSrc {
    const void* p;
    long off;
    int Ws, i64;
    // the sampled value's low byte; *bad is raised by an int64 value outside 0..255
    __device__ __forceinline__ int at(int sy, int sx, int* bad) const {
        const long i = off + (long)sy * Ws + sx;
        if (i64) {
            const long v = ((const long*)p)[i];
            if (v < 0 || v > 255) *bad = 1;
            return (int)(v & 255);
        }
        return ((const unsigned char*)p)[i];
    }
};

__device__ __forceinline__ int pngenc_src_index(int x, double inv, int n) {
    const int i = (int)floor((double)x * inv);
    return i < n - 1 ? i : n - 1;
}

__device__ __forceinline__ int pngenc_paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int pngenc_abs8(int v) {                      // |(int8) v| of a filtered byte
    v &= 255;
    return v < 128 ? v : 256 - v;
}

__global__ __launch_bounds__(PNGENC_THREADS) void pngenc_filter_kernel(const void* __restrict__ src, long src_elems, int src_i64,
                                                                       const PngEncDesc* __restrict__ desc, int max_h, long max_raw,
                                                                       PngEncLayout lay, unsigned char* __restrict__ ws, long out_bytes) {
    __shared__ int s_sum[5];
    __shared__ int s_bad;
    const int img = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
    const PngEncDesc d = desc[img];
    if (!pngenc_fits(d, src_elems, max_h, max_raw, lay.raw_region, out_bytes) || y >= d.Ho) return;
    if (tid < 5) s_sum[tid] = 0;
    if (tid == 5) s_bad = 0;
    __syncthreads();
    const int Wo = d.Wo;
    const double invx = 1.0 / ((double)Wo / (double)d.Ws), invy = 1.0 / ((double)d.Ho / (double)d.Hs);
    PngEncSrc S;
    S.p = src, S.off = d.src_off, S.Ws = d.Ws, S.i64 = src_i64;
    const int sy = pngenc_src_index(y, invy, d.Hs), syu = y > 0 ? pngenc_src_index(y - 1, invy, d.Hs) : 0;
    int bad = 0;
    int sum[5] = {0, 0, 0, 0, 0};
    for (int x = tid; x < Wo; x += PNGENC_THREADS) {                     // trips bounded by Wo <= 65535
        const int sx = pngenc_src_index(x, invx, d.Ws), sxl = x > 0 ? pngenc_src_index(x - 1, invx, d.Ws) : 0;
        const int cur = S.at(sy, sx, &bad);
        const int a = x > 0 ? S.at(sy, sxl, &bad) : 0;
        const int b = y > 0 ? S.at(syu, sx, &bad) : 0;
        const int c = (x > 0 && y > 0) ? S.at(syu, sxl, &bad) : 0;
        sum[0] += pngenc_abs8(cur);
        sum[1] += pngenc_abs8(cur - a);
        sum[2] += pngenc_abs8(cur - b);
        sum[3] += pngenc_abs8(cur - ((a + b) >> 1));
        sum[4] += pngenc_abs8(cur - pngenc_paeth(a, b, c));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        int v = sum[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((tid & 63) == 0) atomicAdd(&s_sum[f], v);                    // integer sums: the order does not matter
    }
    if (bad) s_bad = 1;
    __syncthreads();
    int ft = 0, best = s_sum[0];
#pragma unroll
    for (int f = 1; f < 5; ++f)
        if (s_sum[f] < best) best = s_sum[f], ft = f;
    unsigned char* row = ws + d.raw_off + (long)y * (1 + (long)Wo);
    if (tid == 0) {
        row[0] = (unsigned char)ft;
        if (s_bad) reinterpret_cast<int*>(ws + lay.flag_off)[img] = 1;   // every raiser stores the same 1 into the zeroed word
    }
    for (int x = tid; x < Wo; x += PNGENC_THREADS) {
        const int sx = pngenc_src_index(x, invx, d.Ws), sxl = x > 0 ? pngenc_src_index(x - 1, invx, d.Ws) : 0;
        const int cur = S.at(sy, sx, &bad);
        int p = 0;
        if (ft == 1) {
            p = x > 0 ? S.at(sy, sxl, &bad) : 0;
        } else if (ft == 2) {
            p = y > 0 ? S.at(syu, sx, &bad) : 0;
        } else if (ft >= 3) {
            const int a = x > 0 ? S.at(sy, sxl, &bad) : 0;
            const int b = y > 0 ? S.at(syu, sx, &bad) : 0;
            const int c = (x > 0 && y > 0) ? S.at(syu, sxl, &bad) : 0;
            p = ft == 3 ? (a + b) >> 1 : pngenc_paeth(a, b, c);
        }
        row[1 + x] = (unsigned char)((cur - p) & 255);
    }
}

// ------------------------------------------------------------------------------------------------ chunked fixed-Huffman deflate

// RFC 1951 3.2.5 / 3.2.6 with the fixed codes: the token's bits as they enter the LSB-first stream (Huffman codes bit-reversed, extra
// bits as they are) and their count (at most 31: 8 + 5 + 5 + 13)
__device__ __forceinline__ unsigned pngenc_rev(unsigned code, int n) { return __brev(code) >> (32 - n); }

__device__ __forceinline__ unsigned pngenc_literal(unsigned b, int* nbits) {
    if (b < 144u) {
        *nbits = 8;
        return pngenc_rev(0x30u + b, 8);
    }
    *nbits = 9;
    return pngenc_rev(0x190u + (b - 144u), 9);
}

// dist_bits / dist_n: the distance's code and extra bits, already in stream order
__device__ __forceinline__ unsigned pngenc_match(int len, unsigned dist_bits, int dist_n, int* nbits) {
    int idx, e = 0;
    unsigned ext = 0;
    const int l = len - 3;
    if (len == PNGENC_MAX_LEN) {
        idx = 28;
    } else if (l < 8) {
        idx = l;
    } else {
        e = (31 - __clz(l)) - 2;
        idx = 4 + 4 * e + ((l >> e) & 3);
        ext = (unsigned)l & ((1u << e) - 1u);
    }
    unsigned v;
    int n;
    if (idx < 23) {
        v = pngenc_rev((unsigned)idx + 1u, 7), n = 7;                    // symbols 257..279: 7 bits, 0000001..0010111
    } else {
        v = pngenc_rev(0xC0u + (unsigned)(idx - 23), 8), n = 8;          // symbols 280..285: 8 bits, 11000000..
    }
    v |= ext << n, n += e;
    v |= dist_bits << n, n += dist_n;
    *nbits = n;
    return v;
}

__device__ __forceinline__ unsigned pngenc_dist(int dist, int* nbits) {
    const int dd = dist - 1;
    int code, e = 0;
    if (dd < 4) {
        code = dd;
    } else {
        e = (31 - __clz(dd)) - 1;
        code = 2 * e + 2 + ((dd >> e) & 1);
    }
    *nbits = 5 + e;
    return pngenc_rev((unsigned)code, 5) | (((unsigned)dd & ((1u << e) - 1u)) << 5);
}

#define PNGENC_STEP_MASK 0x1FFu        // s_step: the greedy step of the position (1 = a literal, else the match length)
#define PNGENC_TOKEN 0x4000u           //         the parse starts a token here
#define PNGENC_ROW 0x8000u             //         the match uses the distance S

struct PngEncParse {                   // what the token parse of one chunk leaves in LDS
    unsigned char raw[PNGENC_CHUNK];
    unsigned short step[PNGENC_CHUNK];
    unsigned short m1[PNGENC_THREADS], mS[PNGENC_THREADS];
    unsigned long long a, b;           // the chunk's Adler-32 partial sums (ADLER only)
};

struct PngEncLds {
    PngEncParse P;
    unsigned span[PNGENC_SPAN_WORDS];
    unsigned long long scan[4];
};

// the run of ones that starts at bit i of the owner's mask m, continued through the following masks while they are all ones (stops at 258)
__device__ __forceinline__ int pngenc_carry(const unsigned short* masks, int t) {
    int run = 0;
    for (int k = t + 1; k < PNGENC_THREADS && run < PNGENC_MAX_LEN; ++k) {      // at most 17 trips
        const unsigned m = masks[k];
        if (m == 0xFFFFu) {
            run += 16;
        } else {
            run += __builtin_ctz(~m);
            break;
        }
    }
    return run;
}

__device__ __forceinline__ int pngenc_run(unsigned m, int i, int carry) {
    const unsigned r = (~m >> i) & (0xFFFFu >> i);
    return r ? __builtin_ctz(r) : (16 - i) + carry;
}

// The token parse of one chunk, shared by the fixed-code and the dynamic-code kernels: the chunk into LDS, the equality masks, the carry,
// the greedy step of every position and the one-lane walk that flags the token starts in P.step.  ADLER: also the chunk's Adler-32
// partial sums in P.a / P.b.  Called by the whole workgroup; ends with a barrier.
template <bool ADLER>
__device__ __forceinline__ void pngenc_parse(PngEncParse& P, const unsigned char* __restrict__ raw, long c0, int n, long rawn, int S,
                                             bool use_row) {
    const int tid = threadIdx.x, p0 = tid * 16;
    // the chunk into LDS; raw_off and c0 are multiples of 16 and the raw region is padded to 16 bytes
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p0 < n) v = *reinterpret_cast<const uint4*>(raw + c0 + p0);
    *reinterpret_cast<uint4*>(&P.raw[p0]) = v;
    if (tid == 0) P.a = 0, P.b = 0;
    __syncthreads();

    // equality masks of the thread's 16 positions
    unsigned m1 = 0, mS = 0;
    {
        int prev = p0 > 0 ? P.raw[p0 - 1] : (c0 > 0 ? raw[c0 - 1] : -1);
        unsigned long long a = 0, b = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + i;
            if (p < n) {
                const int x = P.raw[p];
                const long g = c0 + p;
                if (x == prev) m1 |= 1u << i;
                if (use_row && g >= S && raw[g - S] == x) mS |= 1u << i;
                prev = x;
                if (ADLER) a += (unsigned)x, b += (unsigned long long)x * (unsigned long long)(rawn - g);
            }
        }
        P.m1[tid] = (unsigned short)m1;
        P.mS[tid] = (unsigned short)mS;
        if (ADLER) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64), b += __shfl_xor(b, o, 64);
            if ((tid & 63) == 0) atomicAdd(&P.a, a), atomicAdd(&P.b, b);
        }
    }
    __syncthreads();

    // the greedy step of every position
    {
        const int carry1 = pngenc_carry(P.m1, tid), carryS = pngenc_carry(P.mS, tid);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int l1 = pngenc_run(m1, i, carry1), lS = pngenc_run(mS, i, carryS);
            l1 = l1 < PNGENC_MAX_LEN ? l1 : PNGENC_MAX_LEN;
            lS = lS < PNGENC_MAX_LEN ? lS : PNGENC_MAX_LEN;
            const bool row = lS > l1;
            const int len = row ? lS : l1;
            P.step[p0 + i] = (unsigned short)(len >= 3 ? (unsigned)len | (row ? PNGENC_ROW : 0u) : 1u);
        }
    }
    __syncthreads();

    // one lane walks the table and flags the token starts: every trip advances by at least one byte
    if (tid == 0) {
        for (int p = 0; p < n;) {
            const unsigned s = P.step[p];
            P.step[p] = (unsigned short)(s | PNGENC_TOKEN);
            p += (int)(s & PNGENC_STEP_MASK);
        }
    }
    __syncthreads();
}

template <bool EMIT>
__global__ __launch_bounds__(PNGENC_THREADS) void pngenc_deflate_kernel(long src_elems, const PngEncDesc* __restrict__ desc, int max_h,
                                                                        long max_raw, PngEncLayout lay, unsigned char* __restrict__ ws,
                                                                        unsigned char* __restrict__ out, long out_bytes,
                                                                        const PngEncResult* __restrict__ result) {
    __shared__ PngEncLds L;
    const int img = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[img];
    if (!pngenc_fits(d, src_elems, max_h, max_raw, lay.raw_region, out_bytes)) return;
    const long rawn = pngenc_raw_bytes(d);
    const long c0 = (long)blockIdx.x * PNGENC_CHUNK;
    if (c0 >= rawn) return;
    if (EMIT && result[img].status != 0) return;
    const int n = (int)(rawn - c0 < PNGENC_CHUNK ? rawn - c0 : PNGENC_CHUNK);      // bytes of this chunk
    const unsigned char* raw = ws + d.raw_off;
    const int S = d.Wo + 1;
    const bool use_row = S <= PNGENC_WINDOW;
    const int p0 = tid * 16;

    pngenc_parse<!EMIT>(L.P, raw, c0, n, rawn, S, use_row);

    // bits of the thread's tokens
    int dist_n = 0, one_n = 0;
    const unsigned dist_bits = pngenc_dist(use_row ? S : 1, &dist_n), one_bits = pngenc_dist(1, &one_n);
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned s = L.P.step[p0 + i];
        if (p0 + i < n && (s & PNGENC_TOKEN)) {
            int nb;
            if ((s & PNGENC_STEP_MASK) == 1u) {
                pngenc_literal(L.P.raw[p0 + i], &nb);
            } else {
                const bool row = (s & PNGENC_ROW) != 0;
                pngenc_match((int)(s & PNGENC_STEP_MASK), row ? dist_bits : one_bits, row ? dist_n : one_n, &nb);
            }
            mine += (unsigned)nb;
        }
    }
    unsigned long long total;
    const unsigned long long before = pngenc_block_scan(mine, L.scan, &total);
    const unsigned bits = 3u + (unsigned)total + 7u;                    // block header, tokens, end of block (0000000)

    if (!EMIT) {
        if (tid == 0) {
            const long ci = (long)img * lay.nchunk + blockIdx.x;
            reinterpret_cast<unsigned*>(ws + lay.bits_off)[ci] = bits;
            unsigned* part = reinterpret_cast<unsigned*>(ws + lay.part_off) + ci * 2;
            part[0] = (unsigned)(L.P.a % PNGENC_ADLER_MOD);
            part[1] = (unsigned)(L.P.b % PNGENC_ADLER_MOD);
        }
        return;
    }

    const unsigned long long bitoff = reinterpret_cast<const unsigned long long*>(ws + lay.off_off)[(long)img * lay.nchunk + blockIdx.x];
    const unsigned sh = (unsigned)(bitoff & 31u);
    const int nw = (int)((sh + bits + 31u) >> 5);                       // <= PNGENC_SPAN_WORDS
    for (int w = tid; w < nw; w += PNGENC_THREADS) L.span[w] = 0;
    __syncthreads();
    if (tid == 0) {                                                      // BFINAL, then BTYPE = 01 (its low bit first)
        const unsigned long long head = (unsigned long long)((c0 + n == rawn ? 1u : 0u) | 2u) << sh;
        atomicOr(&L.span[0], (unsigned)head);
        if (head >> 32) atomicOr(&L.span[1], (unsigned)(head >> 32));
    }
    unsigned pos = sh + 3u + (unsigned)before;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned s = L.P.step[p0 + i];
        if (p0 + i < n && (s & PNGENC_TOKEN)) {
            int nb;
            unsigned val;
            if ((s & PNGENC_STEP_MASK) == 1u) {
                val = pngenc_literal(L.P.raw[p0 + i], &nb);
            } else {
                const bool row = (s & PNGENC_ROW) != 0;
                val = pngenc_match((int)(s & PNGENC_STEP_MASK), row ? dist_bits : one_bits, row ? dist_n : one_n, &nb);
            }
            const unsigned long long wide = (unsigned long long)val << (pos & 31u);
            const unsigned lo = (unsigned)wide, hi = (unsigned)(wide >> 32);
            if (lo) atomicOr(&L.span[pos >> 5], lo);
            if (hi) atomicOr(&L.span[(pos >> 5) + 1], hi);               // (pos + nb - 1) >> 5 < nw
            pos += (unsigned)nb;
        }
    }
    __syncthreads();
    // the scan kernel has checked the whole stream against out_cap: word w0 + nw - 1 holds a bit of this chunk, so it lies inside it
    unsigned* o32 = reinterpret_cast<unsigned*>(out + d.out_off) + (long)(bitoff >> 5);
    for (int w = tid; w < nw; w += PNGENC_THREADS) {
        const unsigned x = L.span[w];
        if (w == 0 || w == nw - 1) {
            if (x) atomicOr(&o32[w], x);
        } else {
            o32[w] = x;
        }
    }
}

__global__ __launch_bounds__(PNGENC_THREADS) void pngenc_scan_kernel(long src_elems, const PngEncDesc* __restrict__ desc, int max_h,
                                                                     long max_raw, PngEncLayout lay, unsigned char* __restrict__ ws,
                                                                     unsigned char* __restrict__ out, long out_bytes,
                                                                     PngEncResult* __restrict__ result) {
    __shared__ unsigned long long s_scan[4];
    __shared__ unsigned long long s_a, s_b;
    const int img = blockIdx.x, tid = threadIdx.x;
    const PngEncDesc d = desc[img];
    PngEncResult r;
    r.stream_bytes = 0, r.status = 0, r.pad = 0;
    if (!pngenc_fits(d, src_elems, max_h, max_raw, lay.raw_region, out_bytes)) {
        r.status = PNGENC_ST_RECORD;
    } else if (reinterpret_cast<const int*>(ws + lay.flag_off)[img] != 0) {
        r.status = PNGENC_ST_RANGE;
    }
    if (r.status != 0) {
        if (tid == 0) result[img] = r;
        return;
    }
    const long rawn = pngenc_raw_bytes(d);
    const long nchunk = (rawn + PNGENC_CHUNK - 1) / PNGENC_CHUNK;       // <= lay.nchunk
    const unsigned* bits = reinterpret_cast<const unsigned*>(ws + lay.bits_off) + (long)img * lay.nchunk;
    const unsigned* part = reinterpret_cast<const unsigned*>(ws + lay.part_off) + (long)img * lay.nchunk * 2;
    unsigned long long* off = reinterpret_cast<unsigned long long*>(ws + lay.off_off) + (long)img * lay.nchunk;
    if (tid == 0) s_a = 0, s_b = 0;
    unsigned long long base = 16, a = 0, b = 0;                          // the chunks follow the two header bytes
    for (long t0 = 0; t0 < nchunk; t0 += PNGENC_THREADS) {
        const long c = t0 + tid;
        const unsigned long long v = c < nchunk ? bits[c] : 0u;
        unsigned long long total;
        const unsigned long long ex = pngenc_block_scan(v, s_scan, &total);
        if (c < nchunk) {
            off[c] = base + ex;
            a += part[2 * c], b += part[2 * c + 1];
        }
        base += total;
    }
    atomicAdd(&s_a, a);
    atomicAdd(&s_b, b);
    __syncthreads();
    const long tb = (long)((base + 7) >> 3);                             // the trailer follows the last block's byte
    r.stream_bytes = tb + 4;
    if (r.stream_bytes > d.out_cap) {
        r.stream_bytes = 0, r.status = PNGENC_ST_FULL;
        if (tid == 0) result[img] = r;
        return;
    }
    // the words more than one writer ORs into: every chunk's first and last, and the trailer's (all below out_cap / 4)
    unsigned* o32 = reinterpret_cast<unsigned*>(out + d.out_off);
    for (long c = tid; c < nchunk; c += PNGENC_THREADS) {
        const unsigned long long o = off[c];
        o32[o >> 5] = 0;
        o32[(o + bits[c] - 1) >> 5] = 0;
    }
    if (tid == 0) o32[tb >> 2] = 0, o32[(tb + 3) >> 2] = 0;
    __syncthreads();
    if (tid == 0) {
        const unsigned A = (unsigned)((1ull + s_a) % PNGENC_ADLER_MOD), B = (unsigned)(((unsigned long long)rawn + s_b) % PNGENC_ADLER_MOD);
        const unsigned adler = (B << 16) | A;
        atomicOr(&o32[0], 0x0178u);                                      // CMF 78, FLG 01: deflate, 32 KB window, fastest
        for (int k = 0; k < 4; ++k) atomicOr(&o32[(tb + k) >> 2], ((adler >> (24 - 8 * k)) & 255u) << (8 * ((tb + k) & 3)));
        result[img] = r;
    }
}

// ------------------------------------------------------------------------------------------------ dynamic-Huffman blocks
//
// hn_png_encode_dyn (restated in tests/png_enc_dyn_ref.py): the same filter, parse and scan, but one deflate block spans PNGDYN_BLOCK
// chunks and is written with a Huffman code built from its own tokens when that is strictly smaller than the fixed code.
//   pngdyn_hist_kernel   one workgroup per chunk: the parse, then the counts of the 286 literal/length symbols (LDS integer atomics), the
//                        sum of extra bits, the number of matches, the chunk's fixed-code token bits and its Adler-32 partial sums.
//   pngdyn_code_kernel   one workgroup per block: sums its chunks' counts (+ one end of block), builds the literal/length code (<= 15
//                        bits) and the code-length code (<= 7 bits), the header bits, every chunk's bit count under both codes, and the
//                        choice; it leaves the chunk bit counts where the scan reads them and the block's symbol table (the fixed code's
//                        when that won), distance entries and header bits in the block record.  Sorting and code assignment are ranks
//                        computed by all threads; the two-queue merge (<= 285 steps), the limiter and the run-length coding (<= 316
//                        lengths) run on one lane, LDS only, every loop bounded by the alphabet size.
//   pngenc_scan_kernel   as it is: a block's header rides in its first chunk's bit count, the end of block in its last one's.
//   pngdyn_emit_kernel   one workgroup per chunk: the parse again, every token from the block's table in LDS.  A token can be 34 bits
//                        (15 + 5 + 1 + 13): the length part and the distance part are ORed in separately, each at most 20 bits.

#define PNGDYN_BLOCK 16                // chunks per deflate block
#define PNGDYN_NSYM 286
#define PNGDYN_HIST_WORDS 292          // per chunk: the 286 counts, then extra bits, matches, fixed-code token bits
#define PNGDYN_HDR_WORDS 144           // 3 + 14 + 19 * 3 + 316 * (7 + 7) = 4498 bits at most
#define PNGDYN_T_DIST 288              // block record: [0, 286) the symbols' (length << 16 | bits in stream order); here (bits, count) of
#define PNGDYN_T_HDRBITS 292           //   distance 1 and of distance S; the header's bit count; [296, 440) the header bits
#define PNGDYN_T_HDR 296
#define PNGDYN_BLK_WORDS (PNGDYN_T_HDR + PNGDYN_HDR_WORDS)
#define PNGDYN_SPAN_WORDS ((31 + 15 * PNGENC_CHUNK + 32 * PNGDYN_HDR_WORDS + 15 + 31) / 32 + 1)

struct PngDynLayout {                  // ws: the fixed path's layout, then per chunk its counts and per block its record
    PngEncLayout base;
    long hist_off, blk_off, nblock, total;
};

__host__ __device__ inline PngDynLayout pngdyn_layout(long n, long max_raw) {
    PngDynLayout l;
    l.base = pngenc_layout(n, max_raw);
    l.nblock = (l.base.nchunk + PNGDYN_BLOCK - 1) / PNGDYN_BLOCK;
    l.hist_off = (l.base.total + 15) & ~15L;
    l.blk_off = l.hist_off + n * l.base.nchunk * PNGDYN_HIST_WORDS * 4;
    l.total = l.blk_off + n * l.nblock * PNGDYN_BLK_WORDS * 4;
    return l;
}

// the length symbol's index (symbol 257 + idx), its extra bits and their count
__device__ __forceinline__ int pngdyn_len_index(int len, int* e, unsigned* ext) {
    const int l = len - 3;
    *e = 0, *ext = 0;
    if (len == PNGENC_MAX_LEN) return 28;
    if (l < 8) return l;
    const int k = (31 - __clz(l)) - 2;
    *e = k, *ext = (unsigned)l & ((1u << k) - 1u);
    return 4 + 4 * k + ((l >> k) & 3);
}

struct PngDynHistLds {
    PngEncParse P;
    unsigned hist[PNGDYN_HIST_WORDS];
};

__global__ __launch_bounds__(PNGENC_THREADS) void pngdyn_hist_kernel(long src_elems, const PngEncDesc* __restrict__ desc, int max_h,
                                                                     long max_raw, PngDynLayout lay, unsigned char* __restrict__ ws,
                                                                     long out_bytes) {
    __shared__ PngDynHistLds L;
    const int img = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[img];
    if (!pngenc_fits(d, src_elems, max_h, max_raw, lay.base.raw_region, out_bytes)) return;
    const long rawn = pngenc_raw_bytes(d);
    const long c0 = (long)blockIdx.x * PNGENC_CHUNK;
    if (c0 >= rawn) return;
    const int n = (int)(rawn - c0 < PNGENC_CHUNK ? rawn - c0 : PNGENC_CHUNK);
    const unsigned char* raw = ws + d.raw_off;
    const int S = d.Wo + 1;
    const bool use_row = S <= PNGENC_WINDOW;
    const int p0 = tid * 16;
    for (int s = tid; s < PNGDYN_HIST_WORDS; s += PNGENC_THREADS) L.hist[s] = 0;
    pngenc_parse<true>(L.P, raw, c0, n, rawn, S, use_row);               // its barriers order the zeroing before the counting

    int dist_n = 0, one_n = 0;
    const unsigned dist_bits = pngenc_dist(use_row ? S : 1, &dist_n), one_bits = pngenc_dist(1, &one_n);
    unsigned extra = 0, matches = 0, fixed = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned s = L.P.step[p0 + i];
        if (p0 + i < n && (s & PNGENC_TOKEN)) {
            int nb;
            if ((s & PNGENC_STEP_MASK) == 1u) {
                const unsigned b = L.P.raw[p0 + i];
                pngenc_literal(b, &nb);
                atomicAdd(&L.hist[b], 1u);
            } else {
                const bool row = (s & PNGENC_ROW) != 0;
                const int len = (int)(s & PNGENC_STEP_MASK);
                pngenc_match(len, row ? dist_bits : one_bits, row ? dist_n : one_n, &nb);
                int e;
                unsigned ext;
                const int idx = pngdyn_len_index(len, &e, &ext);
                atomicAdd(&L.hist[257 + idx], 1u);
                extra += (unsigned)e + (row ? (unsigned)(dist_n - 5) : 0u);
                matches += 1u;
            }
            fixed += (unsigned)nb;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) extra += __shfl_xor(extra, o, 64), matches += __shfl_xor(matches, o, 64), fixed += __shfl_xor(fixed, o, 64);
    if ((tid & 63) == 0) atomicAdd(&L.hist[286], extra), atomicAdd(&L.hist[287], matches), atomicAdd(&L.hist[288], fixed);
    __syncthreads();
    const long ci = (long)img * lay.base.nchunk + blockIdx.x;
    unsigned* h = reinterpret_cast<unsigned*>(ws + lay.hist_off) + ci * PNGDYN_HIST_WORDS;
    for (int s = tid; s < PNGDYN_HIST_WORDS; s += PNGENC_THREADS) h[s] = L.hist[s];
    if (tid == 0) {
        unsigned* part = reinterpret_cast<unsigned*>(ws + lay.base.part_off) + ci * 2;
        part[0] = (unsigned)(L.P.a % PNGENC_ADLER_MOD);
        part[1] = (unsigned)(L.P.b % PNGENC_ADLER_MOD);
    }
}

struct PngDynHuff {                    // scratch of one code construction
    unsigned weight[2 * PNGDYN_NSYM];
    unsigned short parent[2 * PNGDYN_NSYM], depth[2 * PNGDYN_NSYM], sorted[PNGDYN_NSYM + 2];
    int bl[16], next[16];
    int m;
};

// Code lengths of the n counts in cnt (LDS) -> len (LDS), at most `limit` bits: the used symbols sorted by (count, symbol), a two-queue
// Huffman merge in which a leaf goes before an internal node of equal weight, depths clamped to the limit, the Kraft sum repaired one
// unit a step, and the lengths handed back by (count descending, symbol ascending), shortest first.  One used symbol: length 1.  Then
// the canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream, into code.  Called by the whole workgroup.
__device__ void pngdyn_huffman(const unsigned* cnt, int n, int limit, unsigned char* len, unsigned short* code, PngDynHuff& H) {
    const int tid = threadIdx.x;
    if (tid == 0) H.m = 0;
    __syncthreads();
    for (int s = tid; s < n; s += PNGENC_THREADS) {
        const unsigned c = cnt[s];
        if (c) {
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const unsigned cj = cnt[j];
                rank += (cj && (cj < c || (cj == c && j < s))) ? 1 : 0;
            }
            H.sorted[rank] = (unsigned short)s;                          // ranks are a permutation of 0 .. m - 1
            atomicAdd(&H.m, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int m = H.m;                                               // 1 <= m <= n <= PNGDYN_NSYM
        for (int l = 0; l < 16; ++l) H.bl[l] = 0;
        if (m == 1) {
            H.bl[1] = 1;
        } else if (m > 1) {
            for (int i = 0; i < m; ++i) H.weight[i] = cnt[H.sorted[i]];
            int i = 0, j = m;
            for (int k = m; k < 2 * m - 1; ++k) {                        // nodes [m, k) are internal, in the order they were made
                unsigned w = 0;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    int pick;
                    if (i < m && (j >= k || H.weight[i] <= H.weight[j])) {
                        pick = i++;
                    } else {
                        pick = j++;
                    }
                    w += H.weight[pick];
                    H.parent[pick] = (unsigned short)k;
                }
                H.weight[k] = w;
            }
            H.depth[2 * m - 2] = 0;
            for (int node = 2 * m - 3; node >= 0; --node) H.depth[node] = (unsigned short)(H.depth[H.parent[node]] + 1);
            for (int q = 0; q < m; ++q) {
                const int dq = H.depth[q];
                H.bl[dq < limit ? dq : limit] += 1;
            }
            int over = -(1 << limit);
            for (int l = 1; l <= limit; ++l) over += H.bl[l] << (limit - l);
            for (int t = 0; t < n && over > 0; ++t, --over) {
                H.bl[limit] -= 1;
                int b = limit - 1;
                while (b > 1 && H.bl[b] == 0) --b;
                H.bl[b] -= 1;
                H.bl[b + 1] += 2;
            }
        }
        int c = 0;
        H.next[0] = 0;
        for (int l = 1; l <= limit; ++l) {
            c = (c + H.bl[l - 1]) << 1;
            H.next[l] = c;
        }
    }
    __syncthreads();
    for (int s = tid; s < n; s += PNGENC_THREADS) {
        const unsigned c = cnt[s];
        int l = 0;
        if (c) {
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const unsigned cj = cnt[j];
                rank += (cj && (cj > c || (cj == c && j < s))) ? 1 : 0;
            }
            int acc = 0;
            for (l = 1; l < limit; ++l) {
                acc += H.bl[l];
                if (rank < acc) break;
            }
        }
        len[s] = (unsigned char)l;
    }
    __syncthreads();
    for (int s = tid; s < n; s += PNGENC_THREADS) {
        const int l = len[s];
        unsigned v = 0;
        if (l) {
            int before = 0;
            for (int j = 0; j < s; ++j) before += len[j] == l ? 1 : 0;
            v = pngenc_rev((unsigned)(H.next[l] + before), l);
        }
        code[s] = (unsigned short)v;
    }
    __syncthreads();
}

struct PngDynCodeLds {
    PngDynHuff H;
    unsigned cnt[PNGDYN_NSYM + 2];
    unsigned clcnt[20];
    unsigned char len[PNGDYN_NSYM + 34], cllen[20];                      // len: the literal/length lengths, then the distance lengths
    unsigned short code[PNGDYN_NSYM + 2], clcode[20];
    unsigned short rsym[PNGDYN_NSYM + 34];                               // run-length symbols: symbol | extra value << 8
    unsigned hdr[PNGDYN_HDR_WORDS];
    unsigned dyn[PNGDYN_BLOCK], fix[PNGDYN_BLOCK];
    int nrle, hdr_bits, dynamic;
};

__device__ __forceinline__ void pngdyn_put(unsigned* words, int* pos, unsigned v, int nb) {     // one lane; nb <= 20
    if (((*pos + nb + 31) >> 5) <= PNGDYN_HDR_WORDS) {
        const unsigned long long wide = (unsigned long long)v << (*pos & 31);
        words[*pos >> 5] |= (unsigned)wide;
        if (wide >> 32) words[(*pos >> 5) + 1] |= (unsigned)(wide >> 32);
    }
    *pos += nb;
}

__global__ __launch_bounds__(PNGENC_THREADS) void pngdyn_code_kernel(long src_elems, const PngEncDesc* __restrict__ desc, int max_h,
                                                                     long max_raw, PngDynLayout lay, unsigned char* __restrict__ ws,
                                                                     long out_bytes) {
    __shared__ PngDynCodeLds L;
    const int img = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[img];
    if (!pngenc_fits(d, src_elems, max_h, max_raw, lay.base.raw_region, out_bytes)) return;
    const long rawn = pngenc_raw_bytes(d);
    const int nch = (int)((rawn + PNGENC_CHUNK - 1) / PNGENC_CHUNK);     // <= lay.base.nchunk
    const int b0 = (int)blockIdx.x * PNGDYN_BLOCK;
    if (b0 >= nch) return;
    const int nb = nch - b0 < PNGDYN_BLOCK ? nch - b0 : PNGDYN_BLOCK;    // chunks of this block
    const bool final = b0 + nb == nch;
    const int S = d.Wo + 1;
    const bool use_row = S <= PNGENC_WINDOW;
    const long ci = (long)img * lay.base.nchunk + b0;
    const unsigned* hist = reinterpret_cast<const unsigned*>(ws + lay.hist_off) + ci * PNGDYN_HIST_WORDS;

    for (int s = tid; s < PNGDYN_NSYM; s += PNGENC_THREADS) {
        unsigned c = s == 256 ? 1u : 0u;                                 // one end of block
        for (int k = 0; k < nb; ++k) c += hist[k * PNGDYN_HIST_WORDS + s];
        L.cnt[s] = c;
    }
    for (int w = tid; w < PNGDYN_HDR_WORDS; w += PNGENC_THREADS) L.hdr[w] = 0;
    if (tid < 20) L.clcnt[tid] = 0;
    __syncthreads();
    pngdyn_huffman(L.cnt, PNGDYN_NSYM, 15, L.len, L.code, L.H);

    // the distance code: code 0 for distance 1, the row distance's code (code 1 without row matches); both one bit
    int dist_n = 0;
    const unsigned dist_fixed = pngenc_dist(use_row ? S : 2, &dist_n);
    const int dsym = use_row ? (int)pngenc_rev(dist_fixed & 31u, 5) : 1;  // 1 .. 29
    const int dext_n = use_row ? dist_n - 5 : 0;
    const unsigned dext = use_row ? dist_fixed >> 5 : 0u;

    if (tid == 0) {
        int hlit = PNGDYN_NSYM;
        while (hlit > 257 && L.len[hlit - 1] == 0) --hlit;
        // the distance lengths follow the HLIT literal/length lengths in place: the entries they cover belong to unused symbols
        for (int k = 0; k <= dsym; ++k) L.len[hlit + k] = (k == 0 || k == dsym) ? 1 : 0;
        const int total = hlit + dsym + 1;                               // <= 316
        int nr = 0;
        for (int i = 0; i < total;) {                                    // every trip advances i
            const int v = L.len[i];
            int run = 1;
            while (i + run < total && L.len[i + run] == v) ++run;
            if (v == 0) {
                if (run >= 11) {
                    const int k = run < 138 ? run : 138;
                    L.rsym[nr++] = (unsigned short)(18 | ((k - 11) << 8));
                    i += k;
                } else if (run >= 3) {
                    L.rsym[nr++] = (unsigned short)(17 | ((run - 3) << 8));
                    i += run;
                } else {
                    L.rsym[nr++] = 0;
                    i += 1;
                }
            } else {
                L.rsym[nr++] = (unsigned short)v;
                i += 1;
                for (int r = run - 1; r >= 3;) {
                    const int k = r < 6 ? r : 6;
                    L.rsym[nr++] = (unsigned short)(16 | ((k - 3) << 8));
                    i += k, r -= k;
                }
            }
        }
        L.nrle = nr;                                                     // <= total
        for (int k = 0; k < nr; ++k) L.clcnt[L.rsym[k] & 31] += 1;
        L.hdr_bits = hlit;                                               // handed to the header writer below
    }
    __syncthreads();
    pngdyn_huffman(L.clcnt, 19, 7, L.cllen, L.clcode, L.H);

    if (tid == 0) {
        const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const int hlit = L.hdr_bits;
        int hclen = 19;
        while (hclen > 4 && L.cllen[order[hclen - 1]] == 0) --hclen;
        int pos = 0;
        pngdyn_put(L.hdr, &pos, (final ? 1u : 0u) | 4u, 3);              // BFINAL, BTYPE = 10
        pngdyn_put(L.hdr, &pos, (unsigned)(hlit - 257), 5);
        pngdyn_put(L.hdr, &pos, (unsigned)dsym, 5);                      // HDIST - 1
        pngdyn_put(L.hdr, &pos, (unsigned)(hclen - 4), 4);
        for (int k = 0; k < hclen; ++k) pngdyn_put(L.hdr, &pos, L.cllen[order[k]], 3);
        for (int k = 0; k < L.nrle; ++k) {
            const int sym = L.rsym[k] & 31, ev = L.rsym[k] >> 8, l = L.cllen[sym];
            const int eb = sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0));
            pngdyn_put(L.hdr, &pos, (unsigned)L.clcode[sym] | ((unsigned)ev << l), l + eb);
        }
        L.hdr_bits = pos;
    }
    // every chunk's token bits under the block's code: 16 lanes per chunk
    {
        const int k = tid >> 4, j = tid & 15;
        unsigned sum = 0;
        if (k < nb) {
            const unsigned* h = hist + k * PNGDYN_HIST_WORDS;
            for (int s = j; s < PNGDYN_NSYM; s += 16) sum += h[s] * (unsigned)L.len[s];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (j == 0 && k < PNGDYN_BLOCK) {
            L.dyn[k] = k < nb ? sum + hist[k * PNGDYN_HIST_WORDS + 286] + hist[k * PNGDYN_HIST_WORDS + 287] : 0u;
            L.fix[k] = k < nb ? hist[k * PNGDYN_HIST_WORDS + 288] : 0u;
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned dyn_total = 3u + (unsigned)(L.hdr_bits - 3) + (unsigned)L.len[256], fix_total = 3u + 7u;
        for (int k = 0; k < nb; ++k) dyn_total += L.dyn[k], fix_total += L.fix[k];
        L.dynamic = dyn_total < fix_total ? 1 : 0;                       // a tie goes to the fixed code
    }
    __syncthreads();
    const bool dynamic = L.dynamic != 0;
    unsigned* rec = reinterpret_cast<unsigned*>(ws + lay.blk_off) + ((long)img * lay.nblock + blockIdx.x) * PNGDYN_BLK_WORDS;
    unsigned* bits = reinterpret_cast<unsigned*>(ws + lay.base.bits_off) + ci;
    const unsigned head = dynamic ? (unsigned)L.hdr_bits : 3u, eob = dynamic ? (unsigned)L.len[256] : 7u;
    if (tid < nb) bits[tid] = (dynamic ? L.dyn[tid] : L.fix[tid]) + (tid == 0 ? head : 0u) + (tid == nb - 1 ? eob : 0u);
    for (int s = tid; s < PNGDYN_NSYM; s += PNGENC_THREADS) {
        unsigned v;
        int l;
        if (dynamic) {
            v = L.code[s], l = L.len[s];
        } else if (s < 256) {
            v = pngenc_literal((unsigned)s, &l);
        } else if (s == 256) {
            v = 0, l = 7;
        } else if (s < 280) {
            v = pngenc_rev((unsigned)(s - 256), 7), l = 7;
        } else {
            v = pngenc_rev(0xC0u + (unsigned)(s - 280), 8), l = 8;
        }
        rec[s] = ((unsigned)l << 16) | v;
    }
    for (int w = tid; w < PNGDYN_HDR_WORDS; w += PNGENC_THREADS) rec[PNGDYN_T_HDR + w] = dynamic ? L.hdr[w] : (w == 0 ? ((final ? 1u : 0u) | 2u) : 0u);
    if (tid == 0) {
        int one_n = 0;
        const unsigned one_bits = pngenc_dist(1, &one_n);
        rec[PNGDYN_T_DIST + 0] = dynamic ? 0u : one_bits;
        rec[PNGDYN_T_DIST + 1] = dynamic ? 1u : (unsigned)one_n;
        rec[PNGDYN_T_DIST + 2] = dynamic ? (1u | (dext << 1)) : dist_fixed;
        rec[PNGDYN_T_DIST + 3] = dynamic ? (unsigned)(1 + dext_n) : (unsigned)dist_n;
        rec[PNGDYN_T_HDRBITS] = head;
    }
}

struct PngDynEmitLds {
    PngEncParse P;
    unsigned table[PNGDYN_NSYM + 2];
    unsigned span[PNGDYN_SPAN_WORDS];
    unsigned long long scan[4];
};

__device__ __forceinline__ void pngdyn_or(unsigned* span, unsigned pos, unsigned v) {            // v: at most 20 bits
    const unsigned long long wide = (unsigned long long)v << (pos & 31u);
    const unsigned lo = (unsigned)wide, hi = (unsigned)(wide >> 32);
    if (lo) atomicOr(&span[pos >> 5], lo);
    if (hi) atomicOr(&span[(pos >> 5) + 1], hi);
}

__global__ __launch_bounds__(PNGENC_THREADS) void pngdyn_emit_kernel(long src_elems, const PngEncDesc* __restrict__ desc, int max_h,
                                                                     long max_raw, PngDynLayout lay, unsigned char* __restrict__ ws,
                                                                     unsigned char* __restrict__ out, long out_bytes,
                                                                     const PngEncResult* __restrict__ result) {
    __shared__ PngDynEmitLds L;
    const int img = blockIdx.y, tid = threadIdx.x;
    const PngEncDesc d = desc[img];
    if (!pngenc_fits(d, src_elems, max_h, max_raw, lay.base.raw_region, out_bytes)) return;
    const long rawn = pngenc_raw_bytes(d);
    const long c0 = (long)blockIdx.x * PNGENC_CHUNK;
    if (c0 >= rawn) return;
    if (result[img].status != 0) return;
    const int n = (int)(rawn - c0 < PNGENC_CHUNK ? rawn - c0 : PNGENC_CHUNK);
    const unsigned char* raw = ws + d.raw_off;
    const int S = d.Wo + 1;
    const bool use_row = S <= PNGENC_WINDOW;
    const int p0 = tid * 16;
    const bool first = (blockIdx.x % PNGDYN_BLOCK) == 0;                 // the block's header is this chunk's
    const bool last = (blockIdx.x % PNGDYN_BLOCK) == PNGDYN_BLOCK - 1 || c0 + n == rawn;        // and its end of block this one's
    const unsigned* rec = reinterpret_cast<const unsigned*>(ws + lay.blk_off) + ((long)img * lay.nblock + blockIdx.x / PNGDYN_BLOCK) * PNGDYN_BLK_WORDS;
    for (int s = tid; s < PNGDYN_NSYM; s += PNGENC_THREADS) L.table[s] = rec[s];
    pngenc_parse<false>(L.P, raw, c0, n, rawn, S, use_row);

    const unsigned one_bits = rec[PNGDYN_T_DIST + 0], one_n = rec[PNGDYN_T_DIST + 1], row_bits = rec[PNGDYN_T_DIST + 2], row_n = rec[PNGDYN_T_DIST + 3];
    const unsigned head = first ? rec[PNGDYN_T_HDRBITS] : 0u;            // <= 32 * PNGDYN_HDR_WORDS
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned s = L.P.step[p0 + i];
        if (p0 + i < n && (s & PNGENC_TOKEN)) {
            if ((s & PNGENC_STEP_MASK) == 1u) {
                mine += L.table[L.P.raw[p0 + i]] >> 16;
            } else {
                int e;
                unsigned ext;
                const int idx = pngdyn_len_index((int)(s & PNGENC_STEP_MASK), &e, &ext);
                mine += (L.table[257 + idx] >> 16) + (unsigned)e + ((s & PNGENC_ROW) ? row_n : one_n);
            }
        }
    }
    unsigned long long total;
    const unsigned long long before = pngenc_block_scan(mine, L.scan, &total);
    const unsigned eob = L.table[256];
    const unsigned bits = head + (unsigned)total + (last ? eob >> 16 : 0u);
    const long ci = (long)img * lay.base.nchunk + blockIdx.x;
    // the scan kernel placed and bounded the chunk by the code pass's count: a count that differs is a bug, and nothing is written
    if (bits != reinterpret_cast<const unsigned*>(ws + lay.base.bits_off)[ci]) return;
    const unsigned long long bitoff = reinterpret_cast<const unsigned long long*>(ws + lay.base.off_off)[ci];
    const unsigned sh = (unsigned)(bitoff & 31u);
    const int nw = (int)((sh + bits + 31u) >> 5);
    if (nw > PNGDYN_SPAN_WORDS) return;                                  // 15 bits a byte at most: never
    for (int w = tid; w < nw; w += PNGENC_THREADS) L.span[w] = 0;
    __syncthreads();
    if (first) {
        const int hw = (int)((head + 31u) >> 5);
        for (int w = tid; w < hw; w += PNGENC_THREADS) {                  // bits past `head` in the last word are zero
            const unsigned long long wide = (unsigned long long)rec[PNGDYN_T_HDR + w] << sh;
            if ((unsigned)wide) atomicOr(&L.span[w], (unsigned)wide);
            if (wide >> 32) atomicOr(&L.span[w + 1], (unsigned)(wide >> 32));
        }
    }
    if (last && tid == 0) pngdyn_or(L.span, sh + head + (unsigned)total, eob & 0xFFFFu);
    unsigned pos = sh + head + (unsigned)before;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned s = L.P.step[p0 + i];
        if (p0 + i < n && (s & PNGENC_TOKEN)) {
            if ((s & PNGENC_STEP_MASK) == 1u) {
                const unsigned t = L.table[L.P.raw[p0 + i]];
                pngdyn_or(L.span, pos, t & 0xFFFFu);
                pos += t >> 16;
            } else {
                int e;
                unsigned ext;
                const int idx = pngdyn_len_index((int)(s & PNGENC_STEP_MASK), &e, &ext);
                const unsigned t = L.table[257 + idx], l = t >> 16;
                pngdyn_or(L.span, pos, (t & 0xFFFFu) | (ext << l));      // <= 15 + 5 bits
                pos += l + (unsigned)e;
                const bool row = (s & PNGENC_ROW) != 0;
                pngdyn_or(L.span, pos, row ? row_bits : one_bits);       // <= 5 + 13 bits
                pos += row ? row_n : one_n;
            }
        }
    }
    __syncthreads();
    unsigned* o32 = reinterpret_cast<unsigned*>(out + d.out_off) + (long)(bitoff >> 5);
    for (int w = tid; w < nw; w += PNGENC_THREADS) {
        const unsigned x = L.span[w];
        if (w == 0 || w == nw - 1) {
            if (x) atomicOr(&o32[w], x);
        } else {
            o32[w] = x;
        }
    }
}

}  // namespace

extern "C" int hn_png_enc_chunk_bytes(void) { return PNGENC_CHUNK; }

extern "C" long hn_png_enc_cap_bytes(long raw_bytes) {
    if (raw_bytes <= 0 || raw_bytes >= (1L << 30)) return -1;
    const long blocks = (raw_bytes + PNGENC_CHUNK - 1) / PNGENC_CHUNK;
    return (2 + (9 * raw_bytes + 10 * blocks + 7) / 8 + 4 + 15) & ~15L;
}

extern "C" long hn_png_enc_ws_bytes(int N, long max_raw_bytes) {
    if (N <= 0 || N > 65535 || max_raw_bytes <= 0 || max_raw_bytes >= (1L << 30)) return -1;
    return pngenc_layout(N, max_raw_bytes).total;
}

extern "C" int hn_png_encode(const void* src, long src_elems, int src_is_int64, const void* desc, int N, int max_out_h, long max_raw_bytes,
                             void* ws, long ws_bytes, void* out, long out_bytes, void* result, hipStream_t st) {
    HN_CHECK_ARG(src && desc && ws && out && result && N > 0 && N <= 65535 && src_elems > 0 && (src_is_int64 == 0 || src_is_int64 == 1) &&
                 max_out_h > 0 && max_out_h <= 65535 && max_raw_bytes > 0 && max_raw_bytes < (1L << 30) && out_bytes > 0 &&
                 ((uintptr_t)src & (src_is_int64 ? 7 : 0)) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)out & 3) == 0 &&
                 ((uintptr_t)desc & 7) == 0 && ((uintptr_t)result & 7) == 0 && ws_bytes >= hn_png_enc_ws_bytes(N, max_raw_bytes));
    const PngEncLayout lay = pngenc_layout(N, max_raw_bytes);
    const PngEncDesc* recs = (const PngEncDesc*)desc;
    unsigned char* w = (unsigned char*)ws;
    if (hipMemsetAsync(w + lay.flag_off, 0, (size_t)N * 4, st) != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngenc_filter_kernel, dim3((unsigned)max_out_h, (unsigned)N), dim3(PNGENC_THREADS), 0, st, src, src_elems, src_is_int64,
                       recs, max_out_h, max_raw_bytes, lay, w, out_bytes);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngenc_deflate_kernel<false>, dim3((unsigned)lay.nchunk, (unsigned)N), dim3(PNGENC_THREADS), 0, st, src_elems, recs,
                       max_out_h, max_raw_bytes, lay, w, (unsigned char*)out, out_bytes, (const PngEncResult*)result);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngenc_scan_kernel, dim3((unsigned)N), dim3(PNGENC_THREADS), 0, st, src_elems, recs, max_out_h, max_raw_bytes, lay, w,
                       (unsigned char*)out, out_bytes, (PngEncResult*)result);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngenc_deflate_kernel<true>, dim3((unsigned)lay.nchunk, (unsigned)N), dim3(PNGENC_THREADS), 0, st, src_elems, recs,
                       max_out_h, max_raw_bytes, lay, w, (unsigned char*)out, out_bytes, (const PngEncResult*)result);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_png_enc_block_chunks(void) { return PNGDYN_BLOCK; }

extern "C" long hn_png_enc_dyn_ws_bytes(int N, long max_raw_bytes) {
    if (N <= 0 || N > 65535 || max_raw_bytes <= 0 || max_raw_bytes >= (1L << 30)) return -1;
    return pngdyn_layout(N, max_raw_bytes).total;
}

extern "C" int hn_png_encode_dyn(const void* src, long src_elems, int src_is_int64, const void* desc, int N, int max_out_h, long max_raw_bytes,
                                 void* ws, long ws_bytes, void* out, long out_bytes, void* result, hipStream_t st) {
    HN_CHECK_ARG(src && desc && ws && out && result && N > 0 && N <= 65535 && src_elems > 0 && (src_is_int64 == 0 || src_is_int64 == 1) &&
                 max_out_h > 0 && max_out_h <= 65535 && max_raw_bytes > 0 && max_raw_bytes < (1L << 30) && out_bytes > 0 &&
                 ((uintptr_t)src & (src_is_int64 ? 7 : 0)) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)out & 3) == 0 &&
                 ((uintptr_t)desc & 7) == 0 && ((uintptr_t)result & 7) == 0 && ws_bytes >= hn_png_enc_dyn_ws_bytes(N, max_raw_bytes));
    const PngDynLayout lay = pngdyn_layout(N, max_raw_bytes);
    const PngEncDesc* recs = (const PngEncDesc*)desc;
    unsigned char* w = (unsigned char*)ws;
    const dim3 chunks((unsigned)lay.base.nchunk, (unsigned)N), threads(PNGENC_THREADS);
    if (hipMemsetAsync(w + lay.base.flag_off, 0, (size_t)N * 4, st) != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngenc_filter_kernel, dim3((unsigned)max_out_h, (unsigned)N), threads, 0, st, src, src_elems, src_is_int64, recs,
                       max_out_h, max_raw_bytes, lay.base, w, out_bytes);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngdyn_hist_kernel, chunks, threads, 0, st, src_elems, recs, max_out_h, max_raw_bytes, lay, w, out_bytes);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngdyn_code_kernel, dim3((unsigned)lay.nblock, (unsigned)N), threads, 0, st, src_elems, recs, max_out_h, max_raw_bytes,
                       lay, w, out_bytes);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngenc_scan_kernel, dim3((unsigned)N), threads, 0, st, src_elems, recs, max_out_h, max_raw_bytes, lay.base, w,
                       (unsigned char*)out, out_bytes, (PngEncResult*)result);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(pngdyn_emit_kernel, chunks, threads, 0, st, src_elems, recs, max_out_h, max_raw_bytes, lay, w, (unsigned char*)out,
                       out_bytes, (const PngEncResult*)result);
    HN_LAUNCH_CHECK();
}
