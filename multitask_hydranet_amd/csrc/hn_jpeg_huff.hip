// The JPEG encode's entropy stage on the device (jpeg_encode.entropy_encode_device; semantics in DESIGN.md 4h, restated in numpy by
// tests/jpeg_huff_ref.py): the quantised coefficients hn_jpeg_encode wrote -> every image's byte-stuffed scan, bit for bit what
// hn_jpeg_entropy_encode writes between its header and its EOI.  With the fixed Annex K tables a block's code bits depend on that block and
// on the DC of ONE earlier block, whose index is a function of the geometry alone; where the bits land is a prefix sum; byte stuffing is a
// second one.  So nothing is serial, and no workgroup waits on another: six launches over a ragged batch (grid.y = image), each reading what
// the previous one left in the workspace.
//   huff_count_kernel    one thread per block in scan order (MCU-interleaved; Y in (v, u) order, Cb, Cr): its bit count (uint16) and the
//                        sum / range flag of its tile of HUFF_TILE blocks
//   huff_scan_kernel     one workgroup per image walks the tile sums: 64-bit exclusive bit offsets, the image's total, its status so far;
//                        it zeroes the words of the unstuffed stream that two tiles share (the only ones written with atomicOr)
//   huff_emit_kernel     one workgroup per tile: every thread ORs its block's codes into the tile's span assembled in LDS; whole words go
//                        out with plain stores, the span's first and last word with atomicOr (order-independent: deterministic bytes).
//                        The image's last block pads the last byte with ones.
//   huff_ffcount_kernel  0xFF bytes per chunk of STUFF_CHUNK bytes of the unstuffed stream
//   huff_ffscan_kernel   one workgroup per image: exclusive chunk offsets, the result record {scan_bytes, status}
//   huff_stuff_kernel    one workgroup per chunk: the chunk with a 0x00 after every 0xFF, assembled in LDS, stored at its offset in out
// Status per image: 0, -1 (a descriptor that does not fit the buffers, or a value no baseline table can code: DC difference over 11 bits,
// AC over 10), -4 (the stuffed scan is longer than the image's capacity).  An image with a non-zero status has nothing written to out.
// All integer, exact.
#include "hn_common.h"
#include "hn_jpeg_tables.h"

struct JpegHuffDesc {                  // jpeg_encode.py HUFF_DESC_DTYPE (56 bytes)
    long coef_off;                     // byte offset of the image's coefficients in coefs (multiple of 16)
    long out_off;                      // byte offset of its scan in out
    long out_cap;                      // bytes it may use there
    int W, H, ncomp, hs, vs, mcus_x, mcus_y, pad;
};
static_assert(sizeof(JpegHuffDesc) == 56, "JpegHuffDesc layout is mirrored by jpeg_encode.py");

struct JpegHuffResult {                // jpeg_encode.py HUFF_RESULT_DTYPE (16 bytes)
    long scan_bytes;                   // length of the stuffed, one-padded scan; 0 unless status == 0
    int status, pad;
};

#define HUFF_FULL (-4)
#define HUFF_BAD (-1)
#define HUFF_TILE 128                  // blocks (= threads) per workgroup of the count and emit kernels
#define HUFF_MAX_BLOCK_BITS 1660       // DC: 11 + 11 bits; 63 AC values of 16 + 10 bits
#define HUFF_SPAN_WORDS ((31 + HUFF_TILE * HUFF_MAX_BLOCK_BITS + 7 + 31) / 32 + 1)
#define STUFF_CHUNK 4096               // bytes of the unstuffed stream per workgroup of the stuffing kernels (16 per thread)

namespace {

// (length << 16) | code of every symbol, built from BITS / HUFFVAL at compile time
struct HuffTabs {
    unsigned ac[2][256];
    unsigned dc[2][16];
};
constexpr HuffTabs make_tabs() {
    HuffTabs t{};
    for (int s = 0; s < 2; ++s) {
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < k_ac_bits[s][len - 1]; ++i, ++k) t.ac[s][k_ac_vals[s][k]] = ((unsigned)len << 16) | code++;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < k_dc_bits[s][len - 1]; ++i, ++k) t.dc[s][k_dc_vals[k]] = ((unsigned)len << 16) | code++;
            code <<= 1;
        }
    }
    return t;
}
__device__ const HuffTabs d_tabs = make_tabs();

// the workspace: one slot per image in each array, sized by the batch's largest block count and capacity
struct HuffLayout {
    long tiles, chunks, ustream_bytes;                                   // per image
    long cnt, trec, toff, info, ustream, fcnt, foff, total;              // byte offsets of the arrays; the whole size
};
__host__ __device__ inline HuffLayout huff_layout(int N, long max_blocks, long max_cap) {
    HuffLayout L;
    L.tiles = (max_blocks + HUFF_TILE - 1) / HUFF_TILE;
    L.chunks = (max_cap + STUFF_CHUNK - 1) / STUFF_CHUNK;
    L.ustream_bytes = (max_cap + 15) / 16 * 16 + 16;
    long o = 0;
    L.cnt = o;     o += ((long)N * L.tiles * HUFF_TILE * 2 + 15) / 16 * 16;    // uint16 per block
    L.trec = o;    o += (long)N * L.tiles * 8;                                  // {bits, flag} per tile
    L.toff = o;    o += (long)N * L.tiles * 8;                                  // 64-bit bit offset per tile
    L.info = o;    o += (long)N * 16;                                           // {total bits, status so far} per image
    L.ustream = o; o += (long)N * L.ustream_bytes;
    L.fcnt = o;    o += ((long)N * L.chunks * 4 + 15) / 16 * 16;
    L.foff = o;    o += (long)N * L.chunks * 8;
    L.total = o;
    return L;
}

struct HuffGeom {
    int nc, hs, vs, bpm, mcus_x;
    int rw0, rh0;                      // luma's own size in blocks (chroma planes have no filling blocks: 1x1 sampling)
    int bw0;                           // luma blocks per row of the plane padded to whole MCUs
    long start1, start2;               // first block of the Cb / Cr plane in the coefficient layout
    long nblocks;
    bool ok;
};

__device__ __forceinline__ HuffGeom huff_geom(const JpegHuffDesc& d, long coef_bytes, long out_bytes, long max_blocks, long max_cap) {
    HuffGeom g;
    g.ok = d.W > 0 && d.H > 0 && d.W <= 65535 && d.H <= 65535 && (d.ncomp == 1 || d.ncomp == 3) && (d.hs == 1 || d.hs == 2) &&
           (d.vs == 1 || d.vs == 2) && (d.vs == 1 || d.hs == 2) && (d.ncomp == 3 || (d.hs == 1 && d.vs == 1));
    g.nc = d.ncomp; g.hs = d.hs; g.vs = d.vs; g.mcus_x = d.mcus_x;
    g.nblocks = 0;
    if (!g.ok) return g;
    g.ok = d.mcus_x == (d.W + 8 * d.hs - 1) / (8 * d.hs) && d.mcus_y == (d.H + 8 * d.vs - 1) / (8 * d.vs);
    if (!g.ok) return g;
    g.bpm = d.hs * d.vs + (d.ncomp == 3 ? 2 : 0);
    g.rw0 = (d.W + 7) >> 3;
    g.rh0 = (d.H + 7) >> 3;
    const long mcus = (long)d.mcus_x * d.mcus_y;
    g.bw0 = d.mcus_x * d.hs;
    g.start1 = mcus * d.hs * d.vs;
    g.start2 = g.start1 + mcus;
    g.nblocks = mcus * g.bpm;
    g.ok = d.coef_off >= 0 && (d.coef_off & 15) == 0 && d.coef_off + g.nblocks * 128 <= coef_bytes && g.nblocks <= max_blocks &&
           d.out_off >= 0 && d.out_cap >= 0 && d.out_cap <= max_cap && d.out_off + d.out_cap <= out_bytes;
    return g;
}

// block `idx` of the scan -> its component, whether it is one of the component's own blocks, its index in the coefficient layout, and the
// index of the block whose DC it is predicted from (-1: none, the predictor is 0): the previous REAL block of the component in scan order
__device__ __forceinline__ void huff_locate(const HuffGeom& g, long idx, int& c, bool& real, long& blk, long& prev) {
    const long m = idx / g.bpm;
    const int j = (int)(idx - m * g.bpm), ny = g.hs * g.vs;
    const int my = (int)(m / g.mcus_x), mx = (int)(m - (long)my * g.mcus_x);
    prev = -1;
    if (j >= ny) {
        c = 1 + (j - ny);
        real = true;
        blk = (c == 1 ? g.start1 : g.start2) + m;
        if (m > 0) prev = blk - 1;
        return;
    }
    c = 0;
    const int v = j / g.hs, u = j - v * g.hs;
    const int by = my * g.vs + v, bx = mx * g.hs + u;
    real = by < g.rh0 && bx < g.rw0;
    blk = (long)by * g.bw0 + bx;
    if (!real) return;
    if (u > 0) { prev = blk - 1; return; }
    if (v > 0) { prev = blk - g.bw0 + (min(g.hs, g.rw0 - mx * g.hs) - 1); return; }
    if (m == 0) return;
    const int pmy = mx ? my : my - 1, pmx = mx ? mx - 1 : g.mcus_x - 1;       // the previous MCU: its last real block
    const int nu = min(g.hs, g.rw0 - pmx * g.hs), nv = min(g.vs, g.rh0 - pmy * g.vs);
    prev = (long)(pmy * g.vs + nv - 1) * g.bw0 + pmx * g.hs + nu - 1;
}

__device__ __forceinline__ int bit_size_d(int a) { return a ? 32 - __clz(a) : 0; }

__device__ __forceinline__ int coef_at(const u32x4 (&v)[8], int z) {       // z: natural index, a compile-time constant at every call
    const unsigned w = v[z >> 3][(z >> 1) & 3];
    return (int)(short)((z & 1) ? (w >> 16) : (w & 0xFFFFu));
}

// n <= 32 bits of val (val < 2^n), MSB first, at bit `pos` of a zeroed big-endian word array in LDS
__device__ __forceinline__ void put_bits(unsigned* s, unsigned pos, unsigned val, int n) {
    const unsigned long long x = (unsigned long long)val << (64 - n - (int)(pos & 31u));
    atomicOr(&s[pos >> 5], (unsigned)(x >> 32));
    const unsigned lo = (unsigned)x;
    if (lo) atomicOr(&s[(pos >> 5) + 1], lo);
}

// one real block (hn_jpeg_enc.hip's encode_block): its bit count; EMIT: its bits at `pos` of s_span.  bad: a value outside the tables (the
// count is then meaningless: the image is refused before anything is emitted).
template <bool EMIT>
__device__ __forceinline__ unsigned walk_block(const u32x4 (&v)[8], int pred, const unsigned* __restrict__ s_ac, const unsigned* __restrict__ s_dc,
                                               unsigned* s_span, unsigned pos, bool& bad) {
    const unsigned pos0 = pos;
    const int diff = coef_at(v, 0) - pred;
    int n = bit_size_d(diff < 0 ? -diff : diff);
    if (n > 11) {
        bad = true;
        n = 0;
    }
    unsigned e = s_dc[n];
    {
        const int len = (int)(e >> 16) + n;
        if (EMIT) put_bits(s_span, pos, ((e & 0xFFFFu) << n) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u)), len);
        pos += len;
    }
    const unsigned zrl = s_ac[0xF0];
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int val = coef_at(v, k_zz[k]);
        if (val == 0) {
            ++run;
            continue;
        }
#pragma unroll
        for (int z = 0; z < 3; ++z)                                      // run <= 62: at most three ZRL
            if (run > 15) {
                if (EMIT) put_bits(s_span, pos, zrl & 0xFFFFu, (int)(zrl >> 16));
                pos += zrl >> 16;
                run -= 16;
            }
        n = bit_size_d(val < 0 ? -val : val);
        if (n > 10) {                                                    // (no early exit: the loop stays straight-line code)
            bad = true;
            n = 0;
        }
        e = s_ac[(run << 4) | n];
        const int len = (int)(e >> 16) + n;
        if (EMIT) put_bits(s_span, pos, ((e & 0xFFFFu) << n) | ((unsigned)(val < 0 ? val - 1 : val) & ((1u << n) - 1u)), len);
        pos += len;
        run = 0;
    }
    if (run) {
        e = s_ac[0];
        if (EMIT) put_bits(s_span, pos, e & 0xFFFFu, (int)(e >> 16));
        pos += e >> 16;
    }
    return pos - pos0;
}

// exclusive prefix sum over the NT threads of a workgroup (NT a multiple of 64, at most 1024); total: the sum, in every thread
template <int NT>
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s_w, unsigned& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                                     // s_w may still be read from the previous call
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const unsigned t = s_w[i];
        if (i < w) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

struct HuffInfo {
    unsigned long long total_bits;
    int status, pad;
};

__device__ __forceinline__ void load_tabs(unsigned* s_ac, unsigned* s_dc, int t) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_ac[i] = d_tabs.ac[t][i];
    if (threadIdx.x < 16) s_dc[threadIdx.x] = d_tabs.dc[t][threadIdx.x];
}

}  // namespace

__global__ __launch_bounds__(HUFF_TILE) void huff_count_kernel(const short* __restrict__ coefs, long coef_bytes, const JpegHuffDesc* __restrict__ desc,
                                                               int N, long max_blocks, long max_cap, long out_bytes, unsigned char* __restrict__ ws) {
    __shared__ unsigned s_ac[2][256], s_dc[2][16], s_w[HUFF_TILE / 64], s_bad;
    const int img = blockIdx.y;
    const JpegHuffDesc d = desc[img];
    const HuffGeom g = huff_geom(d, coef_bytes, out_bytes, max_blocks, max_cap);
    if (!g.ok) return;
    const long idx = (long)blockIdx.x * HUFF_TILE + threadIdx.x;
    if ((long)blockIdx.x * HUFF_TILE >= g.nblocks) return;
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    load_tabs(s_ac[0], s_dc[0], 0);
    load_tabs(s_ac[1], s_dc[1], 1);
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    unsigned bits = 0;
    if (idx < g.nblocks) {
        int c;
        bool real;
        long blk, prev;
        huff_locate(g, idx, c, real, blk, prev);
        const int t = c ? 1 : 0;
        if (!real) {
            bits = (s_dc[t][0] >> 16) + (s_ac[t][0] >> 16);
        } else {
            const short* base = coefs + (d.coef_off >> 1);
            const u32x4* p = reinterpret_cast<const u32x4*>(base + blk * 64);
            u32x4 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = p[r];
            const int pred = prev >= 0 ? (int)base[prev * 64] : 0;
            bool bad = false;
            bits = walk_block<false>(v, pred, s_ac[t], s_dc[t], nullptr, 0u, bad);
            if (bad) s_bad = 1u;
        }
        reinterpret_cast<unsigned short*>(ws + L.cnt)[((long)img * L.tiles + blockIdx.x) * HUFF_TILE + threadIdx.x] = (unsigned short)bits;
    }
    unsigned total;
    block_scan<HUFF_TILE>(bits, s_w, total);                             // (its barriers also order s_bad)
    if (threadIdx.x == 0) reinterpret_cast<u32x2*>(ws + L.trec)[(long)img * L.tiles + blockIdx.x] = u32x2{total, s_bad};
}

__global__ __launch_bounds__(256) void huff_scan_kernel(long coef_bytes, const JpegHuffDesc* __restrict__ desc, int N, long max_blocks, long max_cap,
                                                        long out_bytes, unsigned char* __restrict__ ws) {
    __shared__ unsigned s_w[4];
    const int img = blockIdx.x;
    const JpegHuffDesc d = desc[img];
    const HuffGeom g = huff_geom(d, coef_bytes, out_bytes, max_blocks, max_cap);
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    HuffInfo* info = reinterpret_cast<HuffInfo*>(ws + L.info) + img;
    if (!g.ok) {
        if (threadIdx.x == 0) *info = HuffInfo{0ull, HUFF_BAD, 0};
        return;
    }
    const long tiles = (g.nblocks + HUFF_TILE - 1) / HUFF_TILE, uwords = L.ustream_bytes / 4;
    const u32x2* trec = reinterpret_cast<const u32x2*>(ws + L.trec) + (long)img * L.tiles;
    unsigned long long* toff = reinterpret_cast<unsigned long long*>(ws + L.toff) + (long)img * L.tiles;
    unsigned* ustream = reinterpret_cast<unsigned*>(ws + L.ustream + (long)img * L.ustream_bytes);
    unsigned long long carry = 0ull;
    unsigned bad = 0u;
    for (long t0 = 0; t0 < tiles; t0 += 256) {
        const long t = t0 + threadIdx.x;
        u32x2 r = u32x2{0u, 0u};
        if (t < tiles) r = trec[t];
        bad |= r[1];
        unsigned total;
        const unsigned long long off = carry + block_scan<256>(r[0], s_w, total);
        if (t < tiles) {
            toff[t] = off;
            if ((long)(off >> 5) < uwords) ustream[off >> 5] = 0u;       // the word this tile shares with the one before it
        }
        carry += total;
    }
    bad = __syncthreads_or((int)bad);
    if (threadIdx.x == 0) {
        if ((long)(carry >> 5) < uwords) ustream[carry >> 5] = 0u;       // the image's last, padded word
        const unsigned long long ubytes = (carry + 7ull) >> 3;
        *info = HuffInfo{carry, bad ? HUFF_BAD : (ubytes > (unsigned long long)d.out_cap ? HUFF_FULL : 0), 0};
    }
}

__global__ __launch_bounds__(HUFF_TILE) void huff_emit_kernel(const short* __restrict__ coefs, long coef_bytes, const JpegHuffDesc* __restrict__ desc,
                                                              int N, long max_blocks, long max_cap, long out_bytes, unsigned char* __restrict__ ws) {
    __shared__ unsigned s_ac[2][256], s_dc[2][16], s_w[HUFF_TILE / 64];
    __shared__ unsigned s_span[HUFF_SPAN_WORDS];
    const int img = blockIdx.y;
    const JpegHuffDesc d = desc[img];
    const HuffGeom g = huff_geom(d, coef_bytes, out_bytes, max_blocks, max_cap);
    if (!g.ok || (long)blockIdx.x * HUFF_TILE >= g.nblocks) return;
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    const HuffInfo info = reinterpret_cast<const HuffInfo*>(ws + L.info)[img];
    if (info.status != 0) return;
    const long idx = (long)blockIdx.x * HUFF_TILE + threadIdx.x;
    const unsigned long long start = reinterpret_cast<const unsigned long long*>(ws + L.toff)[(long)img * L.tiles + blockIdx.x];
    unsigned bits = 0;
    if (idx < g.nblocks) bits = reinterpret_cast<const unsigned short*>(ws + L.cnt)[((long)img * L.tiles + blockIdx.x) * HUFF_TILE + threadIdx.x];
    unsigned span;
    const unsigned rel = block_scan<HUFF_TILE>(bits, s_w, span);
    const unsigned lead = (unsigned)(start & 31ull);
    const bool last_tile = (long)(blockIdx.x + 1) * HUFF_TILE >= g.nblocks;
    const unsigned padn = last_tile ? (unsigned)((8ull - ((start + span) & 7ull)) & 7ull) : 0u;
    const unsigned end = lead + span + padn;                              // bits of s_span in use
    const unsigned nw = (end + 31u) >> 5;
    for (unsigned i = threadIdx.x; i < nw + 1u; i += HUFF_TILE) s_span[i] = 0u;
    load_tabs(s_ac[0], s_dc[0], 0);
    load_tabs(s_ac[1], s_dc[1], 1);
    __syncthreads();
    if (idx < g.nblocks) {
        int c;
        bool real;
        long blk, prev;
        huff_locate(g, idx, c, real, blk, prev);
        const int t = c ? 1 : 0;
        const unsigned pos = lead + rel;
        if (!real) {
            const unsigned e0 = s_dc[t][0], e1 = s_ac[t][0];
            put_bits(s_span, pos, ((e0 & 0xFFFFu) << (e1 >> 16)) | (e1 & 0xFFFFu), (int)((e0 >> 16) + (e1 >> 16)));
        } else {
            const short* base = coefs + (d.coef_off >> 1);
            const u32x4* p = reinterpret_cast<const u32x4*>(base + blk * 64);
            u32x4 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = p[r];
            const int pred = prev >= 0 ? (int)base[prev * 64] : 0;
            bool bad = false;
            walk_block<true>(v, pred, s_ac[t], s_dc[t], s_span, pos, bad);
        }
        if (padn && idx == g.nblocks - 1) put_bits(s_span, lead + span, (1u << padn) - 1u, (int)padn);
    }
    __syncthreads();
    unsigned* ustream = reinterpret_cast<unsigned*>(ws + L.ustream + (long)img * L.ustream_bytes);
    const long w0 = (long)(start >> 5), uwords = L.ustream_bytes / 4;
    for (unsigned i = threadIdx.x; i < nw; i += HUFF_TILE) {
        if (w0 + i >= uwords) continue;                                   // (status 0 implies the stream fits its slot)
        const unsigned word = __builtin_bswap32(s_span[i]);              // the stream's byte order in memory
        if (i == 0u || (i == nw - 1u && (end & 31u) != 0u)) atomicOr(&ustream[w0 + i], word);
        else ustream[w0 + i] = word;
    }
}

__device__ __forceinline__ unsigned ff_count16(const u32x4& v, long first, long ubytes) {
    unsigned n = 0;
#pragma unroll
    for (int b = 0; b < 16; ++b)
        n += (first + b < ubytes && ((v[b >> 2] >> (8 * (b & 3))) & 255u) == 255u) ? 1u : 0u;
    return n;
}

__global__ __launch_bounds__(256) void huff_ffcount_kernel(int N, long max_blocks, long max_cap, unsigned char* __restrict__ ws) {
    __shared__ unsigned s_w[4];
    const int img = blockIdx.y;
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    const HuffInfo info = reinterpret_cast<const HuffInfo*>(ws + L.info)[img];
    if (info.status != 0) return;
    const long ubytes = (long)((info.total_bits + 7ull) >> 3);
    if ((long)blockIdx.x * STUFF_CHUNK >= ubytes) return;
    const long first = (long)blockIdx.x * STUFF_CHUNK + threadIdx.x * 16;
    unsigned n = 0;
    if (first < ubytes) n = ff_count16(*reinterpret_cast<const u32x4*>(ws + L.ustream + (long)img * L.ustream_bytes + first), first, ubytes);
    unsigned total;
    block_scan<256>(n, s_w, total);
    if (threadIdx.x == 0) reinterpret_cast<unsigned*>(ws + L.fcnt)[(long)img * L.chunks + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void huff_ffscan_kernel(const JpegHuffDesc* __restrict__ desc, int N, long max_blocks, long max_cap,
                                                          unsigned char* __restrict__ ws, JpegHuffResult* __restrict__ result) {
    __shared__ unsigned s_w[4];
    const int img = blockIdx.x;
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    const HuffInfo info = reinterpret_cast<const HuffInfo*>(ws + L.info)[img];
    if (info.status != 0) {
        if (threadIdx.x == 0) result[img] = JpegHuffResult{0L, info.status, 0};
        return;
    }
    const long ubytes = (long)((info.total_bits + 7ull) >> 3), chunks = (ubytes + STUFF_CHUNK - 1) / STUFF_CHUNK;
    const unsigned* fcnt = reinterpret_cast<const unsigned*>(ws + L.fcnt) + (long)img * L.chunks;
    unsigned long long* foff = reinterpret_cast<unsigned long long*>(ws + L.foff) + (long)img * L.chunks;
    unsigned long long carry = 0ull;
    for (long c0 = 0; c0 < chunks; c0 += 256) {
        const long c = c0 + threadIdx.x;
        const unsigned n = c < chunks ? fcnt[c] : 0u;
        unsigned total;
        const unsigned long long off = carry + block_scan<256>(n, s_w, total);
        if (c < chunks) foff[c] = off;
        carry += total;
    }
    if (threadIdx.x == 0) {
        const long need = ubytes + (long)carry;
        result[img] = need > desc[img].out_cap ? JpegHuffResult{0L, HUFF_FULL, 0} : JpegHuffResult{need, 0, 0};
    }
}

__global__ __launch_bounds__(256) void huff_stuff_kernel(const JpegHuffDesc* __restrict__ desc, int N, long max_blocks, long max_cap,
                                                         const unsigned char* __restrict__ ws, const JpegHuffResult* __restrict__ result,
                                                         unsigned char* __restrict__ out, long out_bytes) {
    __shared__ unsigned s_w[4];
    __shared__ unsigned char s_out[2 * STUFF_CHUNK];
    const int img = blockIdx.y;
    const JpegHuffResult res = result[img];
    if (res.status != 0) return;
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    const HuffInfo info = reinterpret_cast<const HuffInfo*>(ws + L.info)[img];
    const long ubytes = (long)((info.total_bits + 7ull) >> 3);
    if ((long)blockIdx.x * STUFF_CHUNK >= ubytes) return;
    const long first = (long)blockIdx.x * STUFF_CHUNK + threadIdx.x * 16;
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    unsigned n = 0;
    if (first < ubytes) {
        v = *reinterpret_cast<const u32x4*>(ws + L.ustream + (long)img * L.ustream_bytes + first);
        n = ff_count16(v, first, ubytes);
    }
    unsigned total;
    unsigned o = threadIdx.x * 16 + block_scan<256>(n, s_w, total);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const unsigned byte = (v[b >> 2] >> (8 * (b & 3))) & 255u;
        if (first + b < ubytes) {
            s_out[o++] = (unsigned char)byte;
            if (byte == 255u) s_out[o++] = 0;
        }
    }
    __syncthreads();
    const JpegHuffDesc d = desc[img];
    const long chunk_bytes = min((long)STUFF_CHUNK, ubytes - (long)blockIdx.x * STUFF_CHUNK) + total;
    const long at = (long)blockIdx.x * STUFF_CHUNK + (long)reinterpret_cast<const unsigned long long*>(ws + L.foff)[(long)img * L.chunks + blockIdx.x];
    for (long i = threadIdx.x; i < chunk_bytes; i += 256) {
        const long pos = at + i;
        if (pos < d.out_cap && d.out_off + pos < out_bytes) out[d.out_off + pos] = s_out[i];    // (status 0: always true)
    }
}

extern "C" long hn_jpeg_huff_ws_bytes(int N, long max_blocks, long max_cap) {
    if (N <= 0 || N > 65535 || max_blocks <= 0 || max_blocks > (1L << 31) - HUFF_TILE || max_cap < 0 || max_cap > (1L << 40)) return -(long)HN_ERR_ARG;
    return huff_layout(N, max_blocks, max_cap).total;
}

extern "C" int hn_jpeg_huff_encode(const void* coefs, long coef_bytes, const void* desc, int N, long max_blocks, long max_cap, void* ws,
                                   long ws_bytes, void* out, long out_bytes, void* result, hipStream_t st) {
    HN_CHECK_ARG(coefs && desc && ws && out && result && coef_bytes > 0 && out_bytes >= 0 && ((uintptr_t)coefs & 15) == 0 && ((uintptr_t)ws & 15) == 0 &&
                 ((uintptr_t)result & 7) == 0);
    const long need = hn_jpeg_huff_ws_bytes(N, max_blocks, max_cap);
    HN_CHECK_ARG(need > 0 && ws_bytes >= need);
    const HuffLayout L = huff_layout(N, max_blocks, max_cap);
    HN_CHECK_ARG(L.tiles <= 0x7FFFFFFFL && L.chunks <= 0x7FFFFFFFL);
    const dim3 gt((unsigned)L.tiles, (unsigned)N), gc((unsigned)(L.chunks > 0 ? L.chunks : 1), (unsigned)N);
    const JpegHuffDesc* dd = (const JpegHuffDesc*)desc;
    unsigned char* w = (unsigned char*)ws;
    hipLaunchKernelGGL(huff_count_kernel, gt, dim3(HUFF_TILE), 0, st, (const short*)coefs, coef_bytes, dd, N, max_blocks, max_cap, out_bytes, w);
    hipLaunchKernelGGL(huff_scan_kernel, dim3((unsigned)N), dim3(256), 0, st, coef_bytes, dd, N, max_blocks, max_cap, out_bytes, w);
    hipLaunchKernelGGL(huff_emit_kernel, gt, dim3(HUFF_TILE), 0, st, (const short*)coefs, coef_bytes, dd, N, max_blocks, max_cap, out_bytes, w);
    hipLaunchKernelGGL(huff_ffcount_kernel, gc, dim3(256), 0, st, N, max_blocks, max_cap, w);
    hipLaunchKernelGGL(huff_ffscan_kernel, dim3((unsigned)N), dim3(256), 0, st, dd, N, max_blocks, max_cap, w, (JpegHuffResult*)result);
    hipLaunchKernelGGL(huff_stuff_kernel, gc, dim3(256), 0, st, dd, N, max_blocks, max_cap, (const unsigned char*)w, (const JpegHuffResult*)result,
                       (unsigned char*)out, out_bytes);
    HN_LAUNCH_CHECK();
}
