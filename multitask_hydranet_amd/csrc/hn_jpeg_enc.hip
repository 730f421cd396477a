// Baseline JPEG encode split between device and host (jpeg_encode.py; semantics in DESIGN.md 4h, restated in integer numpy by
// tests/jpeg_enc_ref.py): the mirror image of hn_jpeg.hip, with the same coefficient layout between the two halves.
//
// Device (one launch over a ragged batch, one JpegEncDesc per image):
//   jpeg_enc_kernel  one workgroup per strip of one MCU row (512 pixels wide, 8 or 16 rows).  The strip's BGR bytes are staged in LDS with
//                    aligned 16-byte loads; libjpeg's 16-bit fixed-point RGB -> YCbCr and its h2v1 / h2v2 down-sampling (alternating bias)
//                    go LDS -> LDS, so the sample planes never reach HBM; then one thread per 8x8 block: jfdctint's accurate integer
//                    forward DCT on samples - 128 and quantisation by q * 8, written as int16 with 16-byte stores in the layout
//                    hn_jpeg_entropy_decode produces (de-zigzagged blocks, plane after plane, raster order of the plane padded to whole
//                    MCUs).  Blocks that only fill an MCU (beyond the component's own width / height in blocks) are written as zeros.
// Host (no HIP runtime call, no allocation, usable without a GPU):
//   hn_jpeg_entropy_encode  coefficients -> a complete JFIF stream (SOI, APP0, DQT, SOF0, DHT with the Annex K tables, one interleaved
//                           SOS, byte stuffing, EOI) into a caller buffer of stated capacity.  The MCU-filling blocks are synthesised as
//                           libjpeg's compress_data does: AC zero, DC of the preceding block.
//   hn_jpeg_write_header    the same stream's bytes before the first scan bit, alone: the device entropy stage (hn_jpeg_huff.hip) writes
//                           the scan, the host the header and EOI.
// All arithmetic is integer and exact.
#include "hn_common.h"
#include "hn_jpeg_tables.h"
#include <string.h>

struct JpegEncHead {                   // the first 48 bytes + tables of hn_jpeg.hip's JpegHead (jpeg.py HEAD_DTYPE, 432 bytes)
    int width, height;
    int ncomp;                         // 1 (greyscale) | 3 (YCbCr)
    int hs, vs;                        // luma sampling factors (chroma is 1x1); 1, 1 for greyscale
    int mcus_x, mcus_y;
    int restart_interval;              // must be 0: restart markers are not written
    long coef_bytes;
    long scan_offset;                  // unused here
    unsigned short qt[3][64];          // natural order; qt[1] == qt[2]
};
static_assert(sizeof(JpegEncHead) == 432, "JpegEncHead is jpeg.py's HEAD_DTYPE");

struct JpegEncDesc {                   // jpeg_encode.py DESC_DTYPE (432 bytes)
    long src_off;                      // byte offset of the image's BGR frame (H x W x 3) in frames
    long coef_off;                     // byte offset of its coefficients in coefs (multiple of 16)
    int W, H, ncomp, hs, vs, mcus_x, mcus_y, pad;
    unsigned short qt[3][64];
};
static_assert(sizeof(JpegEncDesc) == 432, "JpegEncDesc layout is mirrored by jpeg_encode.py");

#define HN_JPEG_ENC_FULL (-4L)         // hn_jpeg_entropy_encode: the capacity is too small

// ---- host: entropy stage -------------------------------------------------------------------------------------------------------------
namespace {

struct EncTab {
    unsigned short code[256];
    unsigned char len[256];            // 0 = the symbol has no code
};

void build_enc(EncTab& t, const unsigned char* bits, const unsigned char* vals) {
    memset(&t, 0, sizeof(t));
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) {
            t.code[vals[k]] = (unsigned short)code++;
            t.len[vals[k]] = (unsigned char)len;
        }
        code <<= 1;
    }
}

// bounded byte sink: nothing is written at or past `cap`; `full` records that something was dropped
struct Sink {
    unsigned char* p;
    long cap, pos;
    bool full;
    unsigned long long acc;
    int nbits;
    inline void byte(unsigned b) {
        if (pos < cap) p[pos++] = (unsigned char)b;
        else full = true;
    }
    inline void be16(unsigned v) { byte(v >> 8); byte(v & 255u); }
    inline void bits(unsigned v, int n) {                                // n <= 32 bits of v, MSB first, with byte stuffing
        acc = (acc << n) | (unsigned long long)v;
        nbits += n;
        while (nbits >= 8) {
            const unsigned b = (unsigned)(acc >> (nbits - 8)) & 255u;
            byte(b);
            if (b == 255u) byte(0);
            nbits -= 8;
        }
    }
    inline void flush() {                                                // pad the last byte with ones
        if (nbits) bits((1u << (8 - nbits)) - 1u, 8 - nbits);
        acc = 0;
        nbits = 0;
    }
};

inline int bit_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

// one block: DC difference against `pred`, then the AC run lengths in zigzag order; false for a value no baseline table can code
inline bool encode_block(Sink& s, const EncTab& dc, const EncTab& ac, const short* blk, int& pred) {
    const int diff = (int)blk[0] - pred;
    pred = blk[0];
    int a = diff < 0 ? -diff : diff, n = bit_size(a);
    if (n > 11) return false;
    s.bits(dc.code[n], dc.len[n]);
    if (n) s.bits((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[k_zz[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            s.bits(ac.code[0xF0], ac.len[0xF0]);
            run -= 16;
        }
        a = v < 0 ? -v : v;
        n = bit_size(a);
        if (n > 10) return false;
        const int sym = (run << 4) | n;
        s.bits(((unsigned)ac.code[sym] << n) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), ac.len[sym] + n);
        run = 0;
    }
    if (run) s.bits(ac.code[0], ac.len[0]);
    return true;
}

inline void dummy_block(Sink& s, const EncTab& dc, const EncTab& ac) {    // DC difference 0, end of block
    s.bits(dc.code[0], dc.len[0]);
    s.bits(ac.code[0], ac.len[0]);
}

void put_dht(Sink& s, int tc_th, const unsigned char* bits, const unsigned char* vals) {
    int n = 0;
    for (int i = 0; i < 16; ++i) n += bits[i];
    s.be16(0xFFC4);
    s.be16(2 + 1 + 16 + n);
    s.byte(tc_th);
    for (int i = 0; i < 16; ++i) s.byte(bits[i]);
    for (int i = 0; i < n; ++i) s.byte(vals[i]);
}

// the header record as both host entry points accept it; false = a bad argument
bool load_head(JpegEncHead& h, const void* head) {
    memcpy(&h, head, sizeof(h));
    const int nc = h.ncomp;
    if (h.width < 1 || h.width > 65535 || h.height < 1 || h.height > 65535 || (nc != 1 && nc != 3) || (h.hs != 1 && h.hs != 2) ||
        (h.vs != 1 && h.vs != 2) || (h.vs == 2 && h.hs != 2) || (nc == 1 && (h.hs != 1 || h.vs != 1)) || h.restart_interval != 0 ||
        h.mcus_x != (h.width + 8 * h.hs - 1) / (8 * h.hs) || h.mcus_y != (h.height + 8 * h.vs - 1) / (8 * h.vs))
        return false;
    const long nblocks = (long)h.mcus_x * h.mcus_y * (h.hs * h.vs + (nc == 3 ? 2 : 0));
    if (h.coef_bytes != nblocks * 128) return false;
    for (int c = 0; c < nc; ++c)
        for (int i = 0; i < 64; ++i)
            if (h.qt[c][i] < 1 || h.qt[c][i] > 255) return false;
    if (nc == 3 && memcmp(h.qt[1], h.qt[2], sizeof(h.qt[1])) != 0) return false;
    return true;
}

// everything before the first scan bit: SOI, APP0, DQT, SOF0, DHT, SOS
void put_header(Sink& s, const JpegEncHead& h) {
    const int nc = h.ncomp;
    s.be16(0xFFD8);
    s.be16(0xFFE0);                                                      // APP0: JFIF 1.01, no units, 1:1, no thumbnail
    s.be16(16);
    s.byte('J'); s.byte('F'); s.byte('I'); s.byte('F'); s.byte(0);
    s.be16(0x0101);
    s.byte(0);
    s.be16(1);
    s.be16(1);
    s.byte(0); s.byte(0);
    for (int t = 0; t < (nc == 3 ? 2 : 1); ++t) {
        s.be16(0xFFDB);
        s.be16(67);
        s.byte(t);
        for (int i = 0; i < 64; ++i) s.byte(h.qt[t][k_zz[i]]);
    }
    s.be16(0xFFC0);
    s.be16(8 + 3 * nc);
    s.byte(8);
    s.be16((unsigned)h.height);
    s.be16((unsigned)h.width);
    s.byte(nc);
    for (int c = 0; c < nc; ++c) {
        s.byte(c + 1);
        s.byte(c == 0 ? ((h.hs << 4) | h.vs) : 0x11);
        s.byte(c ? 1 : 0);
    }
    put_dht(s, 0x00, k_dc_bits[0], k_dc_vals);
    put_dht(s, 0x10, k_ac_bits[0], k_ac_vals[0]);
    if (nc == 3) {
        put_dht(s, 0x01, k_dc_bits[1], k_dc_vals);
        put_dht(s, 0x11, k_ac_bits[1], k_ac_vals[1]);
    }
    s.be16(0xFFDA);
    s.be16(6 + 2 * nc);
    s.byte(nc);
    for (int c = 0; c < nc; ++c) {
        s.byte(c + 1);
        s.byte(c ? 0x11 : 0x00);
    }
    s.byte(0); s.byte(63); s.byte(0);
}

}  // namespace

extern "C" long hn_jpeg_write_header(const void* head, void* out, long capacity) {
    if (!head || !out || capacity < 0) return -(long)HN_ERR_ARG;
    JpegEncHead h;
    if (!load_head(h, head)) return -(long)HN_ERR_ARG;
    Sink s = {(unsigned char*)out, capacity, 0, false, 0ull, 0};
    put_header(s, h);
    return s.full ? HN_JPEG_ENC_FULL : s.pos;
}

extern "C" long hn_jpeg_entropy_encode(const void* coefs, long coef_bytes, const void* head, void* out, long capacity) {
    if (!coefs || !head || !out || capacity < 0) return -(long)HN_ERR_ARG;
    JpegEncHead h;
    if (!load_head(h, head) || coef_bytes < h.coef_bytes) return -(long)HN_ERR_ARG;
    const int nc = h.ncomp;

    Sink s = {(unsigned char*)out, capacity, 0, false, 0ull, 0};
    put_header(s, h);
    if (s.full) return HN_JPEG_ENC_FULL;

    EncTab dc[2], ac[2];
    for (int t = 0; t < 2; ++t) {
        build_enc(dc[t], k_dc_bits[t], k_dc_vals);
        build_enc(ac[t], k_ac_bits[t], k_ac_vals[t]);
    }
    long start[3];
    int bw[3], ch[3], cv[3], rw[3], rh[3];
    long nb = 0;
    for (int c = 0; c < nc; ++c) {
        ch[c] = c ? 1 : h.hs;
        cv[c] = c ? 1 : h.vs;
        bw[c] = h.mcus_x * ch[c];
        start[c] = nb;
        nb += (long)bw[c] * h.mcus_y * cv[c];
        const int cw = c ? (h.width + h.hs - 1) / h.hs : h.width, chh = c ? (h.height + h.vs - 1) / h.vs : h.height;
        rw[c] = (cw + 7) / 8;                                            // the component's own size in blocks: the rest fills MCUs
        rh[c] = (chh + 7) / 8;
    }
    const short* in = (const short*)coefs;
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < h.mcus_y; ++my) {
        for (int mx = 0; mx < h.mcus_x; ++mx)
            for (int c = 0; c < nc; ++c)
                for (int v = 0; v < cv[c]; ++v)
                    for (int u = 0; u < ch[c]; ++u) {
                        const int by = my * cv[c] + v, bx = mx * ch[c] + u;
                        const int t = c ? 1 : 0;
                        if (by >= rh[c] || bx >= rw[c]) {
                            dummy_block(s, dc[t], ac[t]);
                            continue;
                        }
                        if (!encode_block(s, dc[t], ac[t], in + (start[c] + (long)by * bw[c] + bx) * 64, pred[c])) return -(long)HN_ERR_ARG;
                    }
        if (s.full) return HN_JPEG_ENC_FULL;
    }
    s.flush();
    s.be16(0xFFD9);
    return s.full ? HN_JPEG_ENC_FULL : s.pos;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
#define ENC_STRIP 512                  // pixels per strip
#define ENC_CHUNKS 97                  // 16-byte chunks that cover 3 * ENC_STRIP bytes at any alignment
#define ENC_RAWPITCH (ENC_CHUNKS * 16 + 16)

struct EncGeom {
    int bw[3], bh[3];                  // blocks per row / column of each component plane, padded to whole MCUs
    int rw[3], rh[3];                  // of the component itself
    long start[3];
    long nblocks;
};

__device__ __forceinline__ EncGeom enc_geom(const JpegEncDesc& d) {
    EncGeom g;
    g.nblocks = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int hs = c ? 1 : d.hs, vs = c ? 1 : d.vs;
        g.bw[c] = d.mcus_x * hs;
        g.bh[c] = d.mcus_y * vs;
        const int cw = c ? (d.W + d.hs - 1) / d.hs : d.W, ch = c ? (d.H + d.vs - 1) / d.vs : d.H;
        g.rw[c] = (cw + 7) >> 3;
        g.rh[c] = (ch + 7) >> 3;
        g.start[c] = g.nblocks;
        if (c < d.ncomp) g.nblocks += (long)g.bw[c] * g.bh[c];
    }
    return g;
}

// the descriptor's extents against the buffers handed to the entry point (uniform per image): an image that does not fit is left out
__device__ __forceinline__ bool enc_fits(const JpegEncDesc& d, const EncGeom& g, long frames_bytes, long coef_bytes) {
    return d.W > 0 && d.H > 0 && d.W <= 65535 && d.H <= 65535 && (d.ncomp == 1 || d.ncomp == 3) && (d.hs == 1 || d.hs == 2) &&
           (d.vs == 1 || d.vs == 2) && (d.ncomp == 3 || (d.hs == 1 && d.vs == 1)) && d.mcus_x == (d.W + 8 * d.hs - 1) / (8 * d.hs) &&
           d.mcus_y == (d.H + 8 * d.vs - 1) / (8 * d.vs) && d.src_off >= 0 && d.src_off + (long)d.H * d.W * 3 <= frames_bytes &&
           d.coef_off >= 0 && (d.coef_off & 15) == 0 && d.coef_off + g.nblocks * 128 <= coef_bytes;
}

#define JE_0_298631336 2446
#define JE_0_390180644 3196
#define JE_0_541196100 4433
#define JE_0_765366865 6270
#define JE_0_899976223 7373
#define JE_1_175875602 9633
#define JE_1_501321110 12299
#define JE_1_847759065 15137
#define JE_1_961570560 16069
#define JE_2_053119869 16819
#define JE_2_562915447 20995
#define JE_3_072711026 25172

// one 8-point pass of jfdctint.c (jpeg_fdct_islow): the row pass (FIRST: outputs scaled up by 2 bits) or the column pass (descale by 15)
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int d[8], int o[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int SH = FIRST ? 11 : 15;
    constexpr int RND = 1 << (SH - 1);
    if (FIRST) {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * JE_0_541196100;
    o[2] = (z1 + t13 * JE_0_765366865 + RND) >> SH;
    o[6] = (z1 - t12 * JE_1_847759065 + RND) >> SH;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * JE_1_175875602;
    const int a4 = t4 * JE_0_298631336, a5 = t5 * JE_2_053119869, a6 = t6 * JE_3_072711026, a7 = t7 * JE_1_501321110;
    z1 *= -JE_0_899976223;
    z2 *= -JE_2_562915447;
    z3 = z3 * -JE_1_961570560 + z5;
    z4 = z4 * -JE_0_390180644 + z5;
    o[7] = (a4 + z1 + z3 + RND) >> SH;
    o[5] = (a5 + z2 + z4 + RND) >> SH;
    o[3] = (a6 + z2 + z3 + RND) >> SH;
    o[1] = (a7 + z1 + z4 + RND) >> SH;
}

__global__ __launch_bounds__(256) void jpeg_enc_kernel(const unsigned char* __restrict__ frames, long frames_bytes,
                                                       const JpegEncDesc* __restrict__ desc, short* __restrict__ coefs, long coef_bytes) {
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[16][ENC_RAWPITCH];
    __shared__ __attribute__((aligned(16))) unsigned char s_y[16][ENC_STRIP];
    __shared__ __attribute__((aligned(16))) unsigned char s_c[2][8][ENC_STRIP];
    __shared__ unsigned int s_q[3][64];
    __shared__ int s_shift[16];
    const JpegEncDesc& d = desc[blockIdx.z];
    const EncGeom g = enc_geom(d);
    if (!enc_fits(d, g, frames_bytes, coef_bytes)) return;
    const int W = d.W, H = d.H, hs = d.hs, vs = d.vs, my = blockIdx.y, x0 = blockIdx.x * ENC_STRIP;
    if (my >= d.mcus_y || x0 >= W) return;                              // (x0 < the padded width implies x0 < W: x0 is a multiple of 16)
    const int tid = threadIdx.x;
    const int rows = 8 * vs, nx = min(ENC_STRIP, W - x0), wpad = min(ENC_STRIP, d.mcus_x * 8 * hs - x0);
    if (tid < 192) s_q[tid >> 6][tid & 63] = (unsigned)d.qt[tid >> 6][tid & 63] * 8u;

    // stage the strip's BGR bytes: every row as the aligned 16-byte chunks that cover it (row `rows` beyond the image repeat the last one)
    for (int i = tid; i < rows * ENC_CHUNKS; i += 256) {
        const int r = i / ENC_CHUNKS, k = i - r * ENC_CHUNKS;
        const long g0 = d.src_off + ((long)min(my * rows + r, H - 1) * W + x0) * 3;
        const long a0 = g0 & ~15L;
        const int shift = (int)(g0 - a0);
        if (k == 0) s_shift[r] = shift;
        if (k * 16 >= shift + nx * 3) continue;
        const long a = a0 + 16L * k;
        u32x4 v;
        if (a + 16 <= frames_bytes) {
            v = *reinterpret_cast<const u32x4*>(frames + a);
        } else {                                                         // the buffer's last, partial chunk
            v = u32x4{0u, 0u, 0u, 0u};
            for (int b = 0; b < 16; ++b)
                if (a + b < frames_bytes) v[b >> 2] |= (unsigned)frames[a + b] << (8 * (b & 3));
        }
        *reinterpret_cast<u32x4*>(&s_raw[r][k * 16]) = v;
    }
    __syncthreads();

    // colour conversion + down-sampling, one unit of hs x vs pixels at a time; columns beyond the image repeat the last pixel
    const int ucols = wpad / hs;
    if (d.ncomp == 1) {
        for (int i = tid; i < 8 * wpad; i += 256) {
            const int r = i / wpad, x = i - r * wpad;
            s_y[r][x] = s_raw[r][s_shift[r] + min(x, nx - 1) * 3];
        }
    } else {
        for (int i = tid; i < 8 * ucols; i += 256) {
            const int uy = i / ucols, ux = i - uy * ucols;
            int cb = 0, cr = 0;
            for (int dy = 0; dy < vs; ++dy) {
                const int r = uy * vs + dy;
                const unsigned char* row = &s_raw[r][s_shift[r]];
                for (int dx = 0; dx < hs; ++dx) {
                    const int x = ux * hs + dx;
                    const unsigned char* p = row + min(x, nx - 1) * 3;
                    const int B = p[0], G = p[1], R = p[2];
                    // jccolor.c: FIX(0.29900) = 19595, FIX(0.58700) = 38470, FIX(0.11400) = 7471, FIX(0.16874) = 11059, FIX(0.33126) = 21709,
                    // FIX(0.50000) = 32768, FIX(0.41869) = 27439, FIX(0.08131) = 5329; ONE_HALF = 32768, CBCR_OFFSET = 128 << 16
                    s_y[r][x] = (unsigned char)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                    cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                    cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
                }
            }
            if (hs == 2) {
                const int bias = vs == 2 ? 1 + (ux & 1) : (ux & 1), sh = vs == 2 ? 2 : 1;     // (x0 / 2 is even: the parity is the plane's)
                cb = (cb + bias) >> sh;
                cr = (cr + bias) >> sh;
            }
            s_c[0][uy][ux] = (unsigned char)cb;
            s_c[1][uy][ux] = (unsigned char)cr;
        }
    }
    __syncthreads();

    // one thread per 8x8 block of the strip
    const int ycols = ENC_STRIP / 8, ccols = ENC_STRIP / 8 / hs, ybl = vs * ycols;
    const int total = ybl + (d.ncomp == 3 ? 2 * ccols : 0);
    if (tid >= total) return;
    int c, lrow, lcol;
    if (tid < ybl) { c = 0; lrow = tid / ycols; lcol = tid - lrow * ycols; }
    else { c = 1 + (tid - ybl) / ccols; lrow = 0; lcol = (tid - ybl) % ccols; }
    const int gbx = blockIdx.x * (c ? ccols : ycols) + lcol, gby = my * (c ? 1 : vs) + lrow;
    if (gbx >= g.bw[c]) return;
    u32x4* out = reinterpret_cast<u32x4*>(coefs + (d.coef_off >> 1) + (g.start[c] + (long)gby * g.bw[c] + gbx) * 64);
    if (gbx >= g.rw[c] || gby >= g.rh[c]) {                             // fills an MCU only: the host stage synthesises it
#pragma unroll
        for (int r = 0; r < 8; ++r) out[r] = u32x4{0u, 0u, 0u, 0u};
        return;
    }
    int ws[8][8];
    const int last = c ? (H + vs - 1) / vs - 1 - my * 8 : 7;            // chroma: the DOWN-SAMPLED rows are replicated to the MCU height
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const unsigned char* src = c ? &s_c[c - 1][min(r, last)][lcol * 8] : &s_y[lrow * 8 + r][lcol * 8];
        const u32x2 v = *reinterpret_cast<const u32x2*>(src);
        int a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = (int)((v[k >> 2] >> (8 * (k & 3))) & 255u) - 128;
        fdct8<true>(a, ws[r]);
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int a[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) a[r] = ws[r][col];
        fdct8<false>(a, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][col] = o[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        u32x4 w;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = ws[r][k];
            const unsigned q = s_q[c][r * 8 + k];
            const int m = (int)(((unsigned)(v < 0 ? -v : v) + (q >> 1)) / q);
            const unsigned hv = (unsigned)(v < 0 ? -m : m) & 0xFFFFu;
            if (k & 1) w[k >> 1] |= hv << 16;
            else w[k >> 1] = hv;
        }
        out[r] = w;
    }
}

extern "C" int hn_jpeg_encode(const void* frames, long frames_bytes, const void* desc, int N, int max_mcus_y, int max_wpad, void* coefs,
                              long coef_bytes, hipStream_t st) {
    HN_CHECK_ARG(frames && desc && coefs && N > 0 && N <= 65535 && max_mcus_y > 0 && max_mcus_y <= 65535 && max_wpad > 0 &&
                 max_wpad <= 65536 + 16 && frames_bytes > 0 && coef_bytes > 0 && ((uintptr_t)frames & 15) == 0 && ((uintptr_t)coefs & 15) == 0);
    hipLaunchKernelGGL(jpeg_enc_kernel, dim3((unsigned)((max_wpad + ENC_STRIP - 1) / ENC_STRIP), (unsigned)max_mcus_y, (unsigned)N), dim3(256), 0,
                       st, (const unsigned char*)frames, frames_bytes, (const JpegEncDesc*)desc, (short*)coefs, coef_bytes);
    HN_LAUNCH_CHECK();
}
