// PNG label decode on the device (png.py; semantics in DESIGN.md 4j): every image's zlib stream (the concatenated IDAT payloads, as they
// lie in the file) -> the H x W uint8 map dataset.imread_label returns, element for element.  Three launches, no workgroup waits on another:
//   png_inflate_kernel   one 64-lane workgroup per stream (RFC 1950 / 1951).  The bit position is wave-uniform: every lane carries the same
//                        reader state over a 1 KB slice of the stream staged in LDS.  The code tables (10-bit primary look-up + canonical
//                        first / count / sorted symbols for longer codes) live in LDS and are rebuilt by the whole wave for every block:
//                        per-length ranks by ballot, one lane per symbol fills its table entries.  A literal is one lane's store; a match is
//                        copied by all lanes, 64 bytes per trip, source index start + (i mod distance).  The last 32 KB of output are kept in
//                        an LDS window: matches read ONLY the window (never global memory), behind a __syncthreads() that orders the stores
//                        of earlier symbols before the loads of this one; every byte also goes to the image's raw region in ws.
//   png_adler_kernel     Adler-32 partial sums of the raw bytes, 16 KB per workgroup.
//   png_unfilter_kernel  one 64-lane workgroup per image: folds the partial sums and compares them with the stream's trailer, then undoes the
//                        row filters on a skewed wavefront: lane k works on row y0 + k at column t - k, takes the pixel above from lane
//                        k - 1 (a DPP wave shift of what that lane produced one step earlier) and remembers it as the next step's upper-left
//                        one.  64 rows in flight, passes of 64 rows; lane 63 writes its reconstructed row back to ws, lane 0 of the next
//                        pass reads it behind a barrier.  Channel 0 of every pixel is stored to out.
// Every loop of the inflate is bounded by the stream's bits (every iteration consumes at least one and the position is checked against the
// length before anything is stored) and every store by the image's expected raw size H (1 + W bpp); no address depends on decoded data
// other than through those two checks and the window mask.  An image whose record does not fit the buffers gets PNG_ST_RECORD and
// nothing written.
#include "hn_common.h"

#define PNG_ST_BLOCK_TYPE 1
#define PNG_ST_STORED_LEN 2
#define PNG_ST_CODE_LENGTHS 3
#define PNG_ST_SYMBOL 4
#define PNG_ST_DISTANCE 5
#define PNG_ST_INPUT 6
#define PNG_ST_RAW_SIZE 7
#define PNG_ST_FILTER 8
#define PNG_ST_ADLER 9
#define PNG_ST_ZLIB_HEADER 10
#define PNG_ST_RECORD 11

#define PNG_WINDOW 32768
#define PNG_INBUF 1024                 // bytes of the stream staged in LDS
#define PNG_PRIMARY 10                 // bits of the primary look-up
#define PNG_ADLER_CHUNK 16384
#define PNG_ADLER_MOD 65521u

namespace {

struct PngDesc {                       // png.py DESC_DTYPE
    long idat_off, idat_len;           // the zlib stream inside data (idat_off a multiple of 4)
    long raw_off;                      // the filtered scanlines inside ws (a multiple of 16)
    long out_off;                      // the H x W result inside out
    int W, H, bpp, pad;
};

struct PngInfo {
    unsigned adler, pad[3];
};

struct PngLayout {                     // ws: the raw regions, then one PngInfo per image, then the Adler partial sums
    long raw_region, info_off, part_off, nchunk, total;
};

__host__ __device__ inline PngLayout png_layout(long n, long max_raw) {
    PngLayout l;
    l.raw_region = n * ((max_raw + 15) & ~15L);
    l.info_off = l.raw_region;
    l.part_off = l.info_off + n * (long)sizeof(PngInfo);
    l.nchunk = (max_raw + PNG_ADLER_CHUNK - 1) / PNG_ADLER_CHUNK;
    l.total = l.part_off + n * l.nchunk * 8;
    return l;
}

__device__ __forceinline__ long png_raw_bytes(const PngDesc& d) { return (long)d.H * (1 + (long)d.W * d.bpp); }

// the record's extents against the buffers handed to the entry point (uniform per image)
__device__ __forceinline__ bool png_fits(const PngDesc& d, long data_bytes, long max_idat, long max_raw, long raw_region, long out_bytes) {
    if (!(d.W >= 1 && d.W <= 65535 && d.H >= 1 && d.H <= 65535 && (d.bpp == 1 || d.bpp == 3))) return false;
    const long raw = png_raw_bytes(d);
    return d.idat_off >= 0 && (d.idat_off & 3) == 0 && d.idat_len >= 0 && d.idat_len <= max_idat &&
           ((d.idat_off + d.idat_len + 3) & ~3L) <= data_bytes && raw <= max_raw && d.raw_off >= 0 && (d.raw_off & 15) == 0 &&
           d.raw_off + ((raw + 15) & ~15L) <= raw_region && d.out_off >= 0 && d.out_off + (long)d.H * d.W <= out_bytes;
}

__constant__ unsigned short c_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ unsigned char c_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ unsigned short c_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char c_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ unsigned char c_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one code: look[low PNG_PRIMARY bits of the stream] = symbol << 4 | length for codes up to PNG_PRIMARY bits (0: a longer code or none);
// longer codes canonically: a code of L bits (MSB first) is first[L] + k for the k-th symbol of that length, sorted[offs[L] + k]
struct PngTab {
    unsigned short look[1 << PNG_PRIMARY];
    unsigned short sorted[288];
    unsigned short first[16], count[16], offs[16];
};

struct PngLds {
    PngTab ll, dd, cl;
    unsigned in32[PNG_INBUF / 4];
    unsigned char lens[320];
    unsigned char win[PNG_WINDOW];
};

__device__ __forceinline__ unsigned uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

// LSB-first bit reader, the same in every lane
struct PngReader {
    const unsigned* words;             // data as aligned words
    long base;                         // byte offset of the stream in data (a multiple of 4)
    int n;                             // stream bytes
    int pos;                           // next byte of the stream to take into acc
    int ibase;                         // in32 holds stream bytes [ibase, ibase + PNG_INBUF); a multiple of 4
    unsigned long long acc;
    int avail;
    unsigned* in32;
    int lane;

    // bytes past the end of the stream read as zeros; used() tells them from real ones
    __device__ __forceinline__ void reload() {
        __syncthreads();
        ibase = pos & ~3;
#pragma unroll
        for (int k = 0; k < PNG_INBUF / 256; ++k) {
            const int wi = lane + 64 * k;
            const long off = (long)ibase + 4L * wi;
            unsigned w = 0;
            if (off >= 0 && off < n) {
                w = words[(base + off) >> 2];
                if (off + 4 > n) w &= (1u << (8 * (int)(n - off))) - 1u;
            }
            in32[wi] = w;
        }
        __syncthreads();
    }
    // at least 32 bits in acc afterwards
    __device__ __forceinline__ void refill() {
        if (avail < 32) {
            unsigned idx = (unsigned)(pos - ibase);
            if (idx + 8u > (unsigned)PNG_INBUF) {
                reload();
                idx = (unsigned)(pos - ibase);
            }
            const unsigned w0 = in32[idx >> 2], w1 = in32[(idx >> 2) + 1];
            const unsigned w = uni((unsigned)((((unsigned long long)w1 << 32) | w0) >> (8 * (idx & 3u))));
            acc |= (unsigned long long)w << avail;
            avail += 32;
            pos += 4;
        }
    }
    __device__ __forceinline__ unsigned bits(int k) {                   // k <= 16, after refill()
        const unsigned v = (unsigned)acc & ((1u << k) - 1u);
        acc >>= k;
        avail -= k;
        return v;
    }
    __device__ __forceinline__ long used() const { return (long)pos * 8 - avail; }
    __device__ __forceinline__ bool over() const { return used() > (long)n * 8; }
};

// Builds T from n code lengths (0..15) with the whole wave.  Returns false for an over-subscribed set, or an incomplete one other than
// zlib's exceptions (no code at all, or a single one-bit code, in a litlen / distance set).
__device__ __forceinline__ bool png_build(PngTab& T, const unsigned char* lens, int n, bool is_cl, int lane) {
    unsigned* look32 = reinterpret_cast<unsigned*>(T.look);
    for (int i = lane; i < (1 << PNG_PRIMARY) / 2; i += 64) look32[i] = 0;
    int cnt[16];
#pragma unroll
    for (int L = 0; L < 16; ++L) cnt[L] = 0;
    for (int g = 0; g * 64 < n; ++g) {
        const int s = g * 64 + lane;
        const int l = s < n ? lens[s] : 0;
#pragma unroll
        for (int L = 1; L < 16; ++L) cnt[L] += __popcll(__ballot(l == L));
    }
    int left = 1, maxlen = 0;
    bool oversub = false;
    int first[16], offs[16];
    int code = 0, run = 0;
    first[0] = 0, offs[0] = 0;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
        left = left * 2 - cnt[L];
        if (left < 0) oversub = true, left = 0;
        if (cnt[L]) maxlen = L;
        code = (code + cnt[L - 1]) << 1;
        first[L] = code;
        offs[L] = run;
        run += cnt[L];
    }
    if (oversub || (left > 0 && (is_cl || maxlen > 1))) return false;
    if (lane == 0) {
#pragma unroll
        for (int L = 0; L < 16; ++L) T.first[L] = (unsigned short)first[L], T.count[L] = (unsigned short)cnt[L], T.offs[L] = (unsigned short)offs[L];
    }
    __syncthreads();                                                     // the table is zeroed before it is filled
    int basec[16];
#pragma unroll
    for (int L = 0; L < 16; ++L) basec[L] = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int g = 0; g * 64 < n; ++g) {
        const int s = g * 64 + lane;
        const int l = s < n ? lens[s] : 0;
        int rank = 0, fc = 0, of = 0;
#pragma unroll
        for (int L = 1; L < 16; ++L) {
            const unsigned long long m = __ballot(l == L);
            if (l == L) rank = basec[L] + __popcll(m & lt), fc = first[L], of = offs[L];
            basec[L] += __popcll(m);
        }
        if (l) {
            T.sorted[of + rank] = (unsigned short)s;                    // of + rank < n <= 288
            if (l <= PNG_PRIMARY) {
                const unsigned rev = __brev((unsigned)(fc + rank)) >> (32 - l);
                const unsigned short e = (unsigned short)((s << 4) | l);
                for (unsigned j = rev & ((1u << PNG_PRIMARY) - 1u); j < (1u << PNG_PRIMARY); j += 1u << l) T.look[j] = e;
            }
        }
    }
    __syncthreads();
    return true;
}

// the symbol at the reader's position (after refill()): its length is taken; -1 when no code matches
__device__ __forceinline__ int png_decode(const PngTab& T, PngReader& rd) {
    const unsigned e = uni(T.look[(unsigned)rd.acc & ((1u << PNG_PRIMARY) - 1u)]);
    if (e & 15u) {
        rd.bits((int)(e & 15u));
        return (int)(e >> 4);
    }
    const unsigned rev = __brev((unsigned)rd.acc);
    for (int L = PNG_PRIMARY + 1; L < 16; ++L) {
        const unsigned d = (rev >> (32 - L)) - uni(T.first[L]);
        if (d < uni(T.count[L])) {
            rd.bits(L);
            return (int)uni(T.sorted[(uni(T.offs[L]) + d) % 288u]);
        }
    }
    return -1;
}

// -> 0 or the status; *out_count bytes were written to raw (never more than expect), *trailer is the stream's Adler-32
__device__ int png_inflate(PngLds& S, const void* data, const PngDesc& d, unsigned char* __restrict__ raw, int expect, int lane,
                           unsigned* trailer) {
    PngReader rd;
    rd.words = (const unsigned*)data;
    rd.base = d.idat_off;
    rd.n = (int)d.idat_len;
    rd.pos = 0, rd.acc = 0, rd.avail = 0, rd.in32 = S.in32, rd.lane = lane;
    rd.ibase = -2 * PNG_INBUF;                                          // nothing staged yet
    const unsigned char* bytes = (const unsigned char*)data + d.idat_off;
    if (rd.n < 6) return PNG_ST_INPUT;
    rd.refill();
    const unsigned cmf = rd.bits(8), flg = rd.bits(8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return PNG_ST_ZLIB_HEADER;
    int outpos = 0;
    for (;;) {
        rd.refill();
        const unsigned bfinal = rd.bits(1), btype = rd.bits(2);
        if (rd.over()) return PNG_ST_INPUT;
        if (btype == 3u) return PNG_ST_BLOCK_TYPE;
        if (btype == 0u) {
            rd.bits(rd.avail & 7);
            rd.refill();
            const unsigned len = rd.bits(16), nlen = rd.bits(16);
            if (rd.over()) return PNG_ST_INPUT;
            if ((len ^ 0xFFFFu) != nlen) return PNG_ST_STORED_LEN;
            rd.pos -= rd.avail >> 3;                                    // whole bytes: back to the byte after NLEN
            rd.avail = 0, rd.acc = 0;
            if ((long)rd.pos + len > (long)rd.n) return PNG_ST_INPUT;
            if ((long)outpos + len > (long)expect) return PNG_ST_RAW_SIZE;
            for (int i = lane; i < (int)len; i += 64) {
                const unsigned char b = bytes[rd.pos + i];
                raw[outpos + i] = b;
                S.win[(outpos + i) & (PNG_WINDOW - 1)] = b;
            }
            rd.pos += (int)len;
            outpos += (int)len;
        } else {
            __syncthreads();                                             // the previous block's table reads are done
            if (btype == 1u) {
                for (int i = lane; i < 320; i += 64) S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
                __syncthreads();
                png_build(S.ll, S.lens, 288, false, lane);
                png_build(S.dd, S.lens + 288, 32, false, lane);
            } else {
                rd.refill();
                const int hlit = (int)rd.bits(5) + 257, hdist = (int)rd.bits(5) + 1, hclen = (int)rd.bits(4) + 4;
                if (rd.over()) return PNG_ST_INPUT;
                if (hlit > 286 || hdist > 30) return PNG_ST_CODE_LENGTHS;
                if (lane < 19) S.lens[lane] = 0;
                __syncthreads();
                for (int i = 0; i < hclen; ++i) {
                    rd.refill();
                    const unsigned v = rd.bits(3);
                    if (lane == 0) S.lens[c_clorder[i]] = (unsigned char)v;
                }
                if (rd.over()) return PNG_ST_INPUT;
                __syncthreads();
                if (!png_build(S.cl, S.lens, 19, true, lane)) return PNG_ST_CODE_LENGTHS;
                const int total = hlit + hdist;
                int i = 0;
                unsigned prev = 0;
                while (i < total) {                                      // every trip takes at least one bit
                    rd.refill();
                    const int sym = png_decode(S.cl, rd);
                    if (sym < 0 || sym > 18) return rd.over() ? PNG_ST_INPUT : PNG_ST_CODE_LENGTHS;
                    if (sym < 16) {
                        if (rd.over()) return PNG_ST_INPUT;
                        if (lane == 0) S.lens[i] = (unsigned char)sym;
                        prev = (unsigned)sym;
                        ++i;
                    } else {
                        int rep;
                        unsigned val = 0;
                        if (sym == 16) {
                            rep = 3 + (int)rd.bits(2);
                            val = prev;
                        } else if (sym == 17) {
                            rep = 3 + (int)rd.bits(3);
                        } else {
                            rep = 11 + (int)rd.bits(7);
                        }
                        if (rd.over()) return PNG_ST_INPUT;
                        if ((sym == 16 && i == 0) || i + rep > total) return PNG_ST_CODE_LENGTHS;
                        for (int j = lane; j < rep; j += 64) S.lens[i + j] = (unsigned char)val;
                        prev = val;
                        i += rep;
                    }
                }
                __syncthreads();
                if (uni(S.lens[256]) == 0u) return PNG_ST_CODE_LENGTHS;   // no end-of-block code
                if (!png_build(S.ll, S.lens, hlit, false, lane)) return PNG_ST_CODE_LENGTHS;
                if (!png_build(S.dd, S.lens + hlit, hdist, false, lane)) return PNG_ST_CODE_LENGTHS;
            }
            for (;;) {                                                   // every trip takes at least one bit
                rd.refill();
                int sym = png_decode(S.ll, rd);
                if (rd.over()) return PNG_ST_INPUT;
                if (sym < 0) return PNG_ST_SYMBOL;
                if (sym < 256) {
                    if (outpos >= expect) return PNG_ST_RAW_SIZE;
                    if (lane == 0) {
                        raw[outpos] = (unsigned char)sym;
                        S.win[outpos & (PNG_WINDOW - 1)] = (unsigned char)sym;
                    }
                    ++outpos;
                    continue;
                }
                if (sym == 256) break;
                sym -= 257;
                if (sym >= 29) return PNG_ST_SYMBOL;
                const int len = (int)c_lbase[sym] + (int)rd.bits((int)c_lext[sym]);
                rd.refill();
                const int ds = png_decode(S.dd, rd);
                if (rd.over()) return PNG_ST_INPUT;
                if (ds < 0 || ds >= 30) return PNG_ST_SYMBOL;
                const int dist = (int)c_dbase[ds] + (int)rd.bits((int)c_dext[ds]);
                if (rd.over()) return PNG_ST_INPUT;
                if (dist > outpos) return PNG_ST_DISTANCE;
                if (outpos + len > expect) return PNG_ST_RAW_SIZE;
                // the window stores of earlier symbols (other lanes') before this symbol's loads; the sources all lie before outpos, so
                // the trips of one match need nothing between them
                __syncthreads();
                const int start = outpos - dist;
                for (int i = lane; i < len; i += 64) {
                    const unsigned char b = S.win[(start + (dist >= len ? i : i % dist)) & (PNG_WINDOW - 1)];
                    raw[outpos + i] = b;
                    S.win[(outpos + i) & (PNG_WINDOW - 1)] = b;
                }
                outpos += len;
            }
        }
        if (bfinal) break;
    }
    if (outpos != expect) return PNG_ST_RAW_SIZE;
    const long tb = (rd.used() + 7) >> 3;                                // the trailer follows the last block's byte
    if (tb + 4 > (long)rd.n) return PNG_ST_INPUT;
    *trailer = ((unsigned)bytes[tb] << 24) | ((unsigned)bytes[tb + 1] << 16) | ((unsigned)bytes[tb + 2] << 8) | (unsigned)bytes[tb + 3];
    return 0;
}

__global__ __launch_bounds__(64) void png_inflate_kernel(const void* __restrict__ data, long data_bytes, const PngDesc* __restrict__ desc,
                                                         long max_idat, long max_raw, PngLayout lay, unsigned char* __restrict__ ws,
                                                         long out_bytes, int* __restrict__ status) {
    __shared__ PngLds S;
    const int img = blockIdx.x, lane = threadIdx.x;
    const PngDesc d = desc[img];
    if (!png_fits(d, data_bytes, max_idat, max_raw, lay.raw_region, out_bytes)) {
        if (lane == 0) status[img] = PNG_ST_RECORD;
        return;
    }
    unsigned trailer = 0;
    const int st = png_inflate(S, data, d, ws + d.raw_off, (int)png_raw_bytes(d), lane, &trailer);
    if (lane == 0) {
        status[img] = st;
        reinterpret_cast<PngInfo*>(ws + lay.info_off)[img].adler = trailer;
    }
}

// partial sums of chunk c of image img: a = sum of its bytes, b = sum of byte g times (raw - g), both mod 65521
__global__ __launch_bounds__(256) void png_adler_kernel(long data_bytes, const PngDesc* __restrict__ desc, long max_idat, long max_raw,
                                                        PngLayout lay, unsigned char* __restrict__ ws, long out_bytes,
                                                        const int* __restrict__ status) {
    __shared__ unsigned long long s_a, s_b;
    const int img = blockIdx.y, tid = threadIdx.x;
    const PngDesc d = desc[img];
    if (!png_fits(d, data_bytes, max_idat, max_raw, lay.raw_region, out_bytes) || status[img] != 0) return;
    const long raw = png_raw_bytes(d);
    const long c0 = (long)blockIdx.x * PNG_ADLER_CHUNK;
    if (c0 >= raw) return;
    if (tid == 0) s_a = 0, s_b = 0;
    __syncthreads();
    const unsigned char* p = ws + d.raw_off;
    const long g0 = c0 + tid * 64L;
    unsigned long long a = 0, b = 0;
    for (int q = 0; q < 4; ++q) {
        const long g = g0 + 16 * q;
        if (g + 16 <= raw) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + g);     // raw_off and g are multiples of 16
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned x = (w[j >> 2] >> (8 * (j & 3))) & 255u;
                a += x;
                b += (unsigned long long)x * (unsigned long long)(raw - g - j);
            }
        } else {
            for (long j = g; j < raw && j < g + 16; ++j) {
                const unsigned x = p[j];
                a += x;
                b += (unsigned long long)x * (unsigned long long)(raw - j);
            }
        }
    }
    atomicAdd(&s_a, a);
    atomicAdd(&s_b, b);
    __syncthreads();
    if (tid == 0) {
        unsigned* part = reinterpret_cast<unsigned*>(ws + lay.part_off) + ((long)img * lay.nchunk + blockIdx.x) * 2;
        part[0] = (unsigned)(s_a % PNG_ADLER_MOD);
        part[1] = (unsigned)(s_b % PNG_ADLER_MOD);
    }
}

__device__ __forceinline__ unsigned png_load_px(const unsigned char* p, int bpp) {
    unsigned v = p[0];
    if (bpp == 3) v |= ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    return v;
}

__device__ __forceinline__ unsigned png_recon1(int ft, unsigned x, unsigned a, unsigned b, unsigned c) {
    unsigned p = 0;
    if (ft == 1) {
        p = a;
    } else if (ft == 2) {
        p = b;
    } else if (ft == 3) {
        p = (a + b) >> 1;
    } else if (ft == 4) {
        const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
        p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x + p) & 255u;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(long data_bytes, const PngDesc* __restrict__ desc, long max_idat, long max_raw,
                                                          PngLayout lay, unsigned char* __restrict__ ws, unsigned char* __restrict__ out,
                                                          long out_bytes, int* __restrict__ status) {
    __shared__ unsigned long long s_a, s_b;
    const int img = blockIdx.x, lane = threadIdx.x;
    const PngDesc d = desc[img];
    if (!png_fits(d, data_bytes, max_idat, max_raw, lay.raw_region, out_bytes) || status[img] != 0) return;
    const long rawn = png_raw_bytes(d);
    if (lane == 0) s_a = 0, s_b = 0;
    __syncthreads();
    {
        const unsigned* part = reinterpret_cast<const unsigned*>(ws + lay.part_off) + (long)img * lay.nchunk * 2;
        const long nchunk = (rawn + PNG_ADLER_CHUNK - 1) / PNG_ADLER_CHUNK;
        unsigned long long a = 0, b = 0;
        for (long c = lane; c < nchunk; c += 64) a += part[2 * c], b += part[2 * c + 1];
        atomicAdd(&s_a, a);
        atomicAdd(&s_b, b);
    }
    __syncthreads();
    const unsigned A = (unsigned)((1ull + s_a) % PNG_ADLER_MOD), B = (unsigned)(((unsigned long long)rawn + s_b) % PNG_ADLER_MOD);
    if (((B << 16) | A) != reinterpret_cast<const PngInfo*>(ws + lay.info_off)[img].adler) {
        if (lane == 0) status[img] = PNG_ST_ADLER;
        return;
    }
    const int W = d.W, H = d.H, bpp = d.bpp;
    const long stride = 1 + (long)W * bpp;
    unsigned char* raw = ws + d.raw_off;
    unsigned char* o = out + d.out_off;
    for (int y0 = 0; y0 < H; y0 += 64) {
        __syncthreads();                                                 // lane 63's row of the previous pass is in memory
        const int y = y0 + lane;
        const bool rowok = y < H;
        unsigned char* rp = raw + (long)(rowok ? y : 0) * stride;
        int ft = rowok ? rp[0] : 0;
        if (ft > 4) {
            status[img] = PNG_ST_FILTER;
            ft = 0;
        }
        const bool frommem = lane == 0 && y0 > 0;
        const unsigned char* upr = raw + (long)(frommem ? y - 1 : 0) * stride + 1;
        const bool keep = lane == 63 && y + 1 < H;
        unsigned left = 0, upleft = 0, outv = 0, cur = 0, upcur = 0;
        for (int t = -1; t < W + 63; ++t) {
            // what lane k - 1 produced one step earlier: the pixel above this step's (wave_shr:1)
            const unsigned above = (unsigned)__builtin_amdgcn_update_dpp(0, (int)outv, 0x138, 0xf, 0xf, false);
            const int x = t - lane, xn = x + 1;
            unsigned ld = 0, ldu = 0;
            if (rowok && xn >= 0 && xn < W) {
                ld = png_load_px(rp + 1 + (long)xn * bpp, bpp);
                if (frommem) ldu = png_load_px(upr + (long)xn * bpp, bpp);
            }
            if (rowok && x >= 0 && x < W) {
                const unsigned b = y == 0 ? 0u : (lane == 0 ? upcur : above);
                const unsigned a = x ? left : 0u, c = x ? upleft : 0u;
                unsigned r = png_recon1(ft, cur & 255u, a & 255u, b & 255u, c & 255u);
                if (bpp == 3)
                    r |= (png_recon1(ft, (cur >> 8) & 255u, (a >> 8) & 255u, (b >> 8) & 255u, (c >> 8) & 255u) << 8) |
                         (png_recon1(ft, (cur >> 16) & 255u, (a >> 16) & 255u, (b >> 16) & 255u, (c >> 16) & 255u) << 16);
                o[(long)y * W + x] = (unsigned char)(r & 255u);
                if (keep) {
                    unsigned char* q = rp + 1 + (long)x * bpp;
                    q[0] = (unsigned char)(r & 255u);
                    if (bpp == 3) q[1] = (unsigned char)((r >> 8) & 255u), q[2] = (unsigned char)((r >> 16) & 255u);
                }
                left = r, upleft = b, outv = r;
            }
            cur = ld, upcur = ldu;
        }
    }
}

}  // namespace

extern "C" long hn_png_ws_bytes(int N, long max_idat_bytes, long max_raw_bytes) {
    if (N <= 0 || N > 65535 || max_idat_bytes <= 0 || max_idat_bytes >= (1L << 28) || max_raw_bytes <= 0 || max_raw_bytes >= (1L << 30)) return -1;
    return png_layout(N, max_raw_bytes).total;
}

extern "C" int hn_png_decode(const void* data, long data_bytes, const void* desc, int N, long max_idat_bytes, long max_raw_bytes, void* ws,
                             long ws_bytes, void* out, long out_bytes, void* status, hipStream_t st) {
    HN_CHECK_ARG(data && desc && ws && out && status && N > 0 && N <= 65535 && max_idat_bytes > 0 && max_idat_bytes < (1L << 28) &&
                 max_raw_bytes > 0 && max_raw_bytes < (1L << 30) && data_bytes > 0 && (data_bytes & 3) == 0 && out_bytes > 0 &&
                 ((uintptr_t)data & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)desc & 7) == 0 &&
                 ws_bytes >= hn_png_ws_bytes(N, max_idat_bytes, max_raw_bytes));
    const PngLayout lay = png_layout(N, max_raw_bytes);
    const PngDesc* recs = (const PngDesc*)desc;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)N), dim3(64), 0, st, data, data_bytes, recs, max_idat_bytes, max_raw_bytes, lay,
                       (unsigned char*)ws, out_bytes, (int*)status);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(png_adler_kernel, dim3((unsigned)lay.nchunk, (unsigned)N), dim3(256), 0, st, data_bytes, recs, max_idat_bytes,
                       max_raw_bytes, lay, (unsigned char*)ws, out_bytes, (const int*)status);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)N), dim3(64), 0, st, data_bytes, recs, max_idat_bytes, max_raw_bytes, lay,
                       (unsigned char*)ws, (unsigned char*)out, out_bytes, (int*)status);
    HN_LAUNCH_CHECK();
}
