// Baseline JPEG decode split between host and device (jpeg.py; semantics in DESIGN.md 4g, restated in integer numpy by tests/jpeg_ref.py).
//
// Host (no HIP runtime call, usable without a GPU and from a DataLoader worker):
//   hn_jpeg_parse           marker walk -> JpegHead (geometry, sampling, quantisation tables in natural order, coefficient buffer size)
//   hn_jpeg_entropy_decode  the Huffman stage of the one interleaved scan -> quantised int16 coefficients, de-zigzagged, one 64-entry block
//                           per 8x8 block, component plane after component plane, blocks in raster order of the plane padded to whole MCUs.
//                           Every stream read is checked against the given length and every block against the buffer size.
//   hn_jpeg_scan_prepare    instead of that stage, for the scan decode on the device (hn_jpeg_scan.hip): where the scan lies and the Huffman
//                           tables it selects -> JpegScanRec
// Device (two launches over a ragged batch, one JpegDesc per image):
//   jpeg_idct_kernel   one thread per 8x8 block: dequantise + libjpeg's accurate integer IDCT (jidctint "ISLOW": 13-bit constants, 2 pass-1
//                      bits), +128, clamp -> uint8 sample planes (width = blocks * 8) in the caller's scratch.
//   jpeg_color_kernel  one thread per 4 output pixels: libjpeg's "fancy" triangle chroma up-sampling (h2v1 / h2v2; plain replication when the
//                      chroma plane is at most 2 samples wide, as libjpeg selects), 16-bit fixed-point YCbCr -> RGB, written as BGR uint8
//                      H x W x 3 at the image's offset of the packed frame buffer (augment.pack's layout).
// All arithmetic is integer and exact; dequantised coefficients are assumed to fit 16 bits (any 8-bit JPEG), so 32-bit sums cannot overflow.
#include "hn_common.h"
#include "hn_jpeg_scan.h"
#include <string.h>

// ---- records shared with jpeg.py ---------------------------------------------------------------------------------------------------
struct JpegHead {                      // jpeg.py HEAD_DTYPE (432 bytes)
    int width, height;
    int ncomp;                         // 1 (greyscale) | 3 (YCbCr)
    int hs, vs;                        // luma sampling factors (chroma is 1x1); 1, 1 for greyscale
    int mcus_x, mcus_y;                // MCUs per row / column
    int restart_interval;              // MCUs between RSTn markers, 0 = none
    long coef_bytes;                   // size of the coefficient buffer the caller provides
    long scan_offset;                  // byte offset of the entropy-coded segment
    unsigned short qt[3][64];          // quantisation table of each component, natural (row-major) order
};
static_assert(sizeof(JpegHead) == 432, "JpegHead layout is mirrored by jpeg.py");

struct JpegDesc {                      // jpeg.py DESC_DTYPE (440 bytes)
    long coef_off;                     // byte offset of the image's coefficients in coefs (multiple of 16)
    long plane_off;                    // byte offset of its sample planes in the scratch (multiple of 16)
    long dst_off;                      // byte offset of its BGR frame in dst
    int W, H, ncomp, hs, vs, mcus_x, mcus_y, pad;
    unsigned short qt[3][64];
};
static_assert(sizeof(JpegDesc) == 440, "JpegDesc layout is mirrored by jpeg.py");

static const unsigned char k_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- host: marker walk ---------------------------------------------------------------------------------------------------------------
namespace {

struct HuffTab {
    bool set;
    unsigned char look_n[512], look_v[512];     // 9-bit look-ahead: code length (0 = longer than 9 bits) and symbol
    int maxcode[17];                            // largest code of each length, -1 = none
    int valoff[17];                             // symbol index = code + valoff[length]
    unsigned char vals[256];
};

struct JpegState {
    JpegHead h;
    HuffTab dc[4], ac[4];
    unsigned short q[4][64];
    bool qset[4];
    int td[3], ta[3];
};

inline int be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// BITS / HUFFVAL of one DHT table -> decode tables; false for a code set that is not a prefix code of at most 16 bits
bool build_huff(HuffTab& t, const unsigned char* bits, const unsigned char* vals, int nvals) {
    memset(t.look_n, 0, sizeof(t.look_n));
    memcpy(t.vals, vals, (size_t)nvals);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.valoff[len] = k - code;
        const int cnt = bits[len - 1];
        if (code + cnt > (1 << len)) return false;
        if (len <= 9)
            for (int i = 0; i < cnt; ++i) {
                const int first = (code + i) << (9 - len);
                for (int j = 0; j < (1 << (9 - len)); ++j) {
                    t.look_n[first + j] = (unsigned char)len;
                    t.look_v[first + j] = vals[k + i];
                }
            }
        k += cnt;
        code += cnt;
        t.maxcode[len] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    t.set = true;
    return true;
}

// HN_OK / HN_ERR_ARG (not a well-formed JPEG) / HN_ERR_UNSUPPORTED (outside the supported set)
int parse_stream(const unsigned char* p, long n, JpegState& s) {
    memset(&s, 0, sizeof(s));
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return HN_ERR_ARG;
    long pos = 2;
    bool sof = false, jfif = false, adobe = false;
    int adobe_tf = 0;
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    for (;;) {
        if (pos + 2 > n || p[pos] != 0xFF) return HN_ERR_ARG;
        while (pos + 1 < n && p[pos + 1] == 0xFF) ++pos;                 // fill bytes
        if (pos + 2 > n) return HN_ERR_ARG;
        const int m = p[pos + 1];
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;             // TEM, RSTn: no payload
        if (m == 0xD8 || m == 0xD9 || m == 0x00) return HN_ERR_ARG;      // SOI again, EOI before a scan, a stuffed byte outside a scan
        if (pos + 2 > n) return HN_ERR_ARG;
        const int len = be16(p + pos);
        if (len < 2 || pos + len > n) return HN_ERR_ARG;
        const unsigned char* d = p + pos + 2;
        const int dl = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (sof) return HN_ERR_UNSUPPORTED;
            if (dl < 6) return HN_ERR_ARG;
            const int prec = d[0], H = be16(d + 1), W = be16(d + 3), nc = d[5];
            if (prec != 8 || H == 0) return HN_ERR_UNSUPPORTED;          // 12-bit; a height given later by DNL
            if (W == 0) return HN_ERR_ARG;
            if (nc != 1 && nc != 3) return HN_ERR_UNSUPPORTED;           // CMYK / YCCK, two components
            if (dl < 6 + 3 * nc) return HN_ERR_ARG;
            for (int c = 0; c < nc; ++c) {
                cid[c] = d[6 + 3 * c];
                ch[c] = d[7 + 3 * c] >> 4;
                cv[c] = d[7 + 3 * c] & 15;
                ctq[c] = d[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4 || ctq[c] > 3) return HN_ERR_ARG;
            }
            s.h.width = W;
            s.h.height = H;
            s.h.ncomp = nc;
            sof = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return HN_ERR_UNSUPPORTED;                                   // progressive, lossless, hierarchical, arithmetic (SOFn, DAC)
        } else if (m == 0xDC) {
            return HN_ERR_UNSUPPORTED;                                   // DNL
        } else if (m == 0xC4) {
            int o = 0;
            while (o < dl) {
                if (o + 17 > dl) return HN_ERR_ARG;
                const int tc = d[o] >> 4, th = d[o] & 15;
                if (tc > 1 || th > 3) return HN_ERR_ARG;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += d[o + 1 + i];
                if (cnt > 256 || o + 17 + cnt > dl) return HN_ERR_ARG;
                if (!build_huff(tc ? s.ac[th] : s.dc[th], d + o + 1, d + o + 17, cnt)) return HN_ERR_ARG;
                o += 17 + cnt;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < dl) {
                const int pq = d[o] >> 4, tq = d[o] & 15;
                if (pq > 1 || tq > 3) return HN_ERR_ARG;
                const int sz = pq ? 128 : 64;
                if (o + 1 + sz > dl) return HN_ERR_ARG;
                for (int i = 0; i < 64; ++i)
                    s.q[tq][k_natural[i]] = (unsigned short)(pq ? be16(d + o + 1 + 2 * i) : d[o + 1 + i]);
                s.qset[tq] = true;
                o += 1 + sz;
            }
        } else if (m == 0xDD) {
            if (dl != 2) return HN_ERR_ARG;
            s.h.restart_interval = be16(d);
        } else if (m == 0xE0) {
            if (dl >= 12 && d[0] == 'J' && d[1] == 'F' && d[2] == 'I' && d[3] == 'F' && d[4] == 0) jfif = true;
        } else if (m == 0xEE) {
            if (dl >= 12 && d[0] == 'A' && d[1] == 'd' && d[2] == 'o' && d[3] == 'b' && d[4] == 'e') {
                adobe = true;
                adobe_tf = d[11];
            }
        } else if (m == 0xDA) {
            if (!sof) return HN_ERR_ARG;
            const int nc = s.h.ncomp;
            if (dl < 1) return HN_ERR_ARG;
            const int ns = d[0];
            if (ns < 1 || ns > 4 || dl != 4 + 2 * ns) return HN_ERR_ARG;
            if (ns != nc) return HN_ERR_UNSUPPORTED;                     // more than one scan
            for (int c = 0; c < nc; ++c) {
                if (d[1 + 2 * c] != cid[c]) return HN_ERR_UNSUPPORTED;   // scan components out of frame order
                s.td[c] = d[2 + 2 * c] >> 4;
                s.ta[c] = d[2 + 2 * c] & 15;
                if (s.td[c] > 3 || s.ta[c] > 3) return HN_ERR_ARG;
                if (!s.dc[s.td[c]].set || !s.ac[s.ta[c]].set || !s.qset[ctq[c]]) return HN_ERR_ARG;
                memcpy(s.h.qt[c], s.q[ctq[c]], sizeof(s.h.qt[c]));
            }
            if (d[1 + 2 * ns] != 0 || d[2 + 2 * ns] != 63 || d[3 + 2 * ns] != 0) return HN_ERR_UNSUPPORTED;
            if (nc == 3) {
                // libjpeg's colour-space guess: JFIF says YCbCr; else Adobe's transform flag; else component ids "RGB" mean RGB
                if (!jfif && adobe && adobe_tf != 1) return HN_ERR_UNSUPPORTED;
                if (!jfif && !adobe && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') return HN_ERR_UNSUPPORTED;
                if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return HN_ERR_UNSUPPORTED;
                if (!((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2))) return HN_ERR_UNSUPPORTED;
                s.h.hs = ch[0];
                s.h.vs = cv[0];
            } else {
                s.h.hs = s.h.vs = 1;                                     // a one-component scan is not interleaved: 8x8 MCUs whatever the factors
            }
            s.h.mcus_x = (s.h.width + 8 * s.h.hs - 1) / (8 * s.h.hs);
            s.h.mcus_y = (s.h.height + 8 * s.h.vs - 1) / (8 * s.h.vs);
            const long mcus = (long)s.h.mcus_x * s.h.mcus_y;
            s.h.coef_bytes = mcus * (s.h.hs * s.h.vs + (nc == 3 ? 2 : 0)) * 128;
            s.h.scan_offset = pos + len;
            return HN_OK;
        }
        pos += len;                                                      // APPn, COM and anything else with a length: skipped
    }
}

// MSB-first bit reader over the entropy-coded segment: `acc` is left aligned and holds `avail` real bits (zeros below them);
// it stops feeding at a marker or at the end of the data, and a read past that point fails.
struct Bits {
    const unsigned char* p;
    long n, pos;
    unsigned long long acc;
    int avail;
    bool stop;
    inline void fill() {
        while (avail <= 56 && !stop) {
            if (pos >= n) { stop = true; break; }
            const unsigned b = p[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || p[pos + 1] != 0) { stop = true; break; }
                pos += 2;
            } else {
                pos += 1;
            }
            acc |= (unsigned long long)b << (56 - avail);
            avail += 8;
        }
    }
    inline bool take(int k) {
        if (k > avail) return false;
        acc <<= k;
        avail -= k;
        return true;
    }
};

inline bool decode_sym(Bits& b, const HuffTab& t, int& sym) {
    if (b.avail < 16) b.fill();
    const unsigned idx = (unsigned)(b.acc >> 55);
    const int ln = t.look_n[idx];
    if (ln) {
        sym = t.look_v[idx];
        return b.take(ln);
    }
    for (int len = 10; len <= 16; ++len) {
        const int code = (int)(b.acc >> (64 - len));
        if (code <= t.maxcode[len]) {
            sym = t.vals[code + t.valoff[len]];
            return b.take(len);
        }
    }
    return false;                                                        // a code that is not in the table
}

inline bool receive_extend(Bits& b, int sbits, int& v) {
    if (b.avail < sbits) b.fill();
    const int raw = (int)(b.acc >> (64 - sbits));
    if (!b.take(sbits)) return false;
    v = raw < (1 << (sbits - 1)) ? raw - (1 << sbits) + 1 : raw;
    return true;
}

bool decode_block(Bits& b, const HuffTab& dc, const HuffTab& ac, int& pred, short* out) {
    memset(out, 0, 128);
    int s;
    if (!decode_sym(b, dc, s) || s > 15) return false;
    if (s) {
        int diff;
        if (!receive_extend(b, s, diff)) return false;
        pred += diff;
    }
    out[0] = (short)pred;
    for (int k = 1; k < 64;) {
        int rs;
        if (!decode_sym(b, ac, rs)) return false;
        const int r = rs >> 4, sz = rs & 15;
        if (sz) {
            k += r;
            if (k > 63) return false;
            int v;
            if (!receive_extend(b, sz, v)) return false;
            out[k_natural[k]] = (short)v;
            ++k;
        } else if (r == 15) {
            k += 16;
        } else {
            break;
        }
    }
    return true;
}

}  // namespace

extern "C" int hn_jpeg_parse(const void* data, long len, void* head) {
    HN_CHECK_ARG(data && head && len > 0);
    JpegState s;
    const int rc = parse_stream((const unsigned char*)data, len, s);
    if (rc != HN_OK) return rc;
    memcpy(head, &s.h, sizeof(JpegHead));
    return HN_OK;
}

extern "C" int hn_jpeg_entropy_decode(const void* data, long len, const void* head, void* coefs, long coef_bytes) {
    HN_CHECK_ARG(data && head && coefs && len > 0);
    JpegState s;
    const int rc = parse_stream((const unsigned char*)data, len, s);
    if (rc != HN_OK) return rc;
    HN_CHECK_ARG(memcmp(head, &s.h, sizeof(JpegHead)) == 0 && coef_bytes >= s.h.coef_bytes);     // the header of this very stream
    const JpegHead& h = s.h;
    const int nc = h.ncomp;
    long start[3];
    int bw[3], ch[3], cv[3];
    long nblocks = 0;
    for (int c = 0; c < nc; ++c) {
        ch[c] = c ? 1 : h.hs;
        cv[c] = c ? 1 : h.vs;
        bw[c] = h.mcus_x * ch[c];
        start[c] = nblocks;
        nblocks += (long)bw[c] * h.mcus_y * cv[c];
    }
    HN_CHECK_ARG(nblocks * 128 == h.coef_bytes);
    short* out = (short*)coefs;
    Bits b = {(const unsigned char*)data, len, h.scan_offset, 0ull, 0, false};
    int pred[3] = {0, 0, 0};
    int since = 0, rst = 0;
    for (int my = 0; my < h.mcus_y; ++my)
        for (int mx = 0; mx < h.mcus_x; ++mx) {
            if (h.restart_interval && since == h.restart_interval) {
                // byte align (what is left in the accumulator is padding), then the expected RSTn marker; predictions reset
                while (b.pos + 1 < b.n && b.p[b.pos] == 0xFF && b.p[b.pos + 1] == 0xFF) ++b.pos;
                if (b.pos + 2 > b.n || b.p[b.pos] != 0xFF || b.p[b.pos + 1] != 0xD0 + rst) return HN_ERR_ARG;
                b.pos += 2;
                b.acc = 0;
                b.avail = 0;
                b.stop = false;
                rst = (rst + 1) & 7;
                since = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < nc; ++c)
                for (int v = 0; v < cv[c]; ++v)
                    for (int u = 0; u < ch[c]; ++u) {
                        const long blk = start[c] + ((long)my * cv[c] + v) * bw[c] + (long)mx * ch[c] + u;
                        if (blk < 0 || (blk + 1) * 128 > coef_bytes) return HN_ERR_ARG;
                        if (!decode_block(b, s.dc[s.td[c]], s.ac[s.ta[c]], pred[c], out + blk * 64)) return HN_ERR_ARG;
                    }
            ++since;
        }
    return HN_OK;
}

// The scan of a supported stream, for hn_jpeg_scan_decode: its extent and the decode tables of its components.  The same statuses as
// hn_jpeg_parse; a `head` that is not this stream's is refused.
extern "C" int hn_jpeg_scan_prepare(const void* data, long len, const void* head, void* rec) {
    HN_CHECK_ARG(data && head && rec && len > 0);
    JpegState s;
    const unsigned char* p = (const unsigned char*)data;
    const int rc = parse_stream(p, len, s);
    if (rc != HN_OK) return rc;
    HN_CHECK_ARG(memcmp(head, &s.h, sizeof(JpegHead)) == 0);                                     // the header of this very stream
    JpegScanRec& r = *(JpegScanRec*)rec;
    memset(&r, 0, sizeof(r));
    r.scan_offset = s.h.scan_offset;
    // the scan ends with the first marker that is neither a stuffed 0xFF nor RSTn (EOI in a whole file), or with the data
    long pos = s.h.scan_offset, end = len;
    while (pos < len) {
        const unsigned char* f = (const unsigned char*)memchr(p + pos, 0xFF, (size_t)(len - pos));
        if (!f || f + 1 >= p + len) break;
        pos = f - p;
        const int m = p[pos + 1];
        if (m == 0 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }
        if (m == 0xFF) { pos += 1; continue; }                                                   // a fill byte
        end = pos + 2;
        break;
    }
    r.scan_bytes = end - s.h.scan_offset;
    r.ncomp = s.h.ncomp, r.hs = s.h.hs, r.vs = s.h.vs, r.mcus_x = s.h.mcus_x, r.mcus_y = s.h.mcus_y, r.restart_interval = s.h.restart_interval;
    for (int kind = 0; kind < 2; ++kind) {
        int used[3], n = 0;
        for (int c = 0; c < s.h.ncomp; ++c) {
            const int id = kind ? s.ta[c] : s.td[c];
            int k = 0;
            while (k < n && used[k] != id) ++k;
            if (k == n) {
                used[n++] = id;
                const HuffTab& t = kind ? s.ac[id] : s.dc[id];
                JpegScanHuff& d = kind ? r.ac[k] : r.dc[k];
                memcpy(d.look_n, t.look_n, sizeof(d.look_n));
                memcpy(d.look_v, t.look_v, sizeof(d.look_v));
                memcpy(d.maxcode, t.maxcode, sizeof(d.maxcode));
                memcpy(d.valoff, t.valoff, sizeof(d.valoff));
                memcpy(d.vals, t.vals, sizeof(d.vals));
            }
            (kind ? r.ta : r.td)[c] = k;
        }
    }
    return HN_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
struct JpegGeom {
    int bw[3], bh[3];                  // blocks per row / column of each component plane
    long start[3];                     // first block of each component (also its plane's byte offset / 64)
    long nblocks;
};

__device__ __forceinline__ JpegGeom jpeg_geom(const JpegDesc& d) {
    JpegGeom g;
    g.nblocks = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = d.mcus_x * (c ? 1 : d.hs);
        g.bh[c] = d.mcus_y * (c ? 1 : d.vs);
        g.start[c] = g.nblocks;
        if (c < d.ncomp) g.nblocks += (long)g.bw[c] * g.bh[c];
    }
    return g;
}

// the descriptor's extents against the buffers handed to the entry point (uniform per image): an image that does not fit is left out
__device__ __forceinline__ bool jpeg_fits(const JpegDesc& d, const JpegGeom& g, long coef_bytes, long plane_bytes, long dst_bytes) {
    return d.W > 0 && d.H > 0 && d.mcus_x > 0 && d.mcus_y > 0 && (d.ncomp == 1 || d.ncomp == 3) && (d.hs == 1 || d.hs == 2) &&
           (d.vs == 1 || d.vs == 2) && (long)d.mcus_x * d.hs * 8 >= d.W && (long)d.mcus_y * d.vs * 8 >= d.H &&
           d.coef_off >= 0 && (d.coef_off & 15) == 0 && d.coef_off + g.nblocks * 128 <= coef_bytes &&
           d.plane_off >= 0 && (d.plane_off & 15) == 0 && d.plane_off + g.nblocks * 64 <= plane_bytes &&
           d.dst_off >= 0 && d.dst_off + (long)d.H * d.W * 3 <= dst_bytes;
}

#define JF_0_298631336 2446
#define JF_0_390180644 3196
#define JF_0_541196100 4433
#define JF_0_765366865 6270
#define JF_0_899976223 7373
#define JF_1_175875602 9633
#define JF_1_501321110 12299
#define JF_1_847759065 15137
#define JF_1_961570560 16069
#define JF_2_053119869 16819
#define JF_2_562915447 20995
#define JF_3_072711026 25172

// one 8-point pass of jidctint.c (jpeg_idct_islow): o[k] = DESCALE(., SHIFT)
template <int SHIFT>
__device__ __forceinline__ void idct8(const int d[8], int o[8]) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * JF_0_541196100;
    int tmp2 = z1 + z3 * (-JF_1_847759065);
    int tmp3 = z1 + z2 * JF_0_765366865;
    int tmp0 = (d[0] + d[4]) * (1 << 13);
    int tmp1 = (d[0] - d[4]) * (1 << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7];
    tmp1 = d[5];
    tmp2 = d[3];
    tmp3 = d[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * JF_1_175875602;
    tmp0 *= JF_0_298631336;
    tmp1 *= JF_2_053119869;
    tmp2 *= JF_3_072711026;
    tmp3 *= JF_1_501321110;
    z1 *= -JF_0_899976223;
    z2 *= -JF_2_562915447;
    z3 *= -JF_1_961570560;
    z4 *= -JF_0_390180644;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int rnd = 1 << (SHIFT - 1);
    o[0] = (tmp10 + tmp3 + rnd) >> SHIFT;
    o[7] = (tmp10 - tmp3 + rnd) >> SHIFT;
    o[1] = (tmp11 + tmp2 + rnd) >> SHIFT;
    o[6] = (tmp11 - tmp2 + rnd) >> SHIFT;
    o[2] = (tmp12 + tmp1 + rnd) >> SHIFT;
    o[5] = (tmp12 - tmp1 + rnd) >> SHIFT;
    o[3] = (tmp13 + tmp0 + rnd) >> SHIFT;
    o[4] = (tmp13 - tmp0 + rnd) >> SHIFT;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coefs, long coef_bytes, const JpegDesc* __restrict__ desc,
                                                        unsigned char* __restrict__ planes, long plane_bytes, long dst_bytes) {
    __shared__ unsigned short s_q[3][64];
    const JpegDesc& d = desc[blockIdx.y];
    const JpegGeom g = jpeg_geom(d);
    if (!jpeg_fits(d, g, coef_bytes, plane_bytes, dst_bytes)) return;
    if ((long)blockIdx.x * 256 >= g.nblocks) return;
    if (threadIdx.x < 192) s_q[threadIdx.x >> 6][threadIdx.x & 63] = d.qt[threadIdx.x >> 6][threadIdx.x & 63];
    __syncthreads();
    const long blk = (long)blockIdx.x * 256 + threadIdx.x;
    if (blk >= g.nblocks) return;
    const int c = (d.ncomp == 3 && blk >= g.start[1]) ? (blk >= g.start[2] ? 2 : 1) : 0;
    const long rel = blk - g.start[c];
    const int by = (int)(rel / g.bw[c]), bx = (int)(rel - (long)by * g.bw[c]);
    const u32x4* in = reinterpret_cast<const u32x4*>(coefs + (d.coef_off >> 1) + blk * 64);
    int ws[8][8];                                                        // [row][column] after pass 1
    int q[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const u32x4 v = in[r];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[r][2 * k] = (int)(short)(v[k] & 0xFFFFu) * (int)s_q[c][r * 8 + 2 * k];
            q[r][2 * k + 1] = (int)(short)(v[k] >> 16) * (int)s_q[c][r * 8 + 2 * k + 1];
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {                                  // pass 1: columns, results scaled up by 2^2
        int a[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) a[r] = q[r][col];
        idct8<11>(a, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][col] = o[r];
    }
    unsigned char* out = planes + d.plane_off + g.start[c] * 64 + ((long)by * 8) * ((long)g.bw[c] * 8) + (long)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                                        // pass 2: rows, descale by 2^(13 + 2 + 3), level shift, clamp
        int o[8];
        idct8<18>(ws[r], o);
        u32x2 w;
        w[0] = clamp255(o[0] + 128) | (clamp255(o[1] + 128) << 8) | (clamp255(o[2] + 128) << 16) | (clamp255(o[3] + 128) << 24);
        w[1] = clamp255(o[4] + 128) | (clamp255(o[5] + 128) << 8) | (clamp255(o[6] + 128) << 16) | (clamp255(o[7] + 128) << 24);
        *reinterpret_cast<u32x2*>(out + (long)r * g.bw[c] * 8) = w;
    }
}

// chroma sample of output pixel (x, y) from plane p (row pitch `pitch`, real size cw x chh), libjpeg's up-sampling for the image's factors
__device__ __forceinline__ int jpeg_chroma(const unsigned char* __restrict__ p, int pitch, int cw, int chh, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(long)y * pitch + x];
    const int i = x >> 1;
    if (cw <= 2) return p[(long)(vs == 2 ? y >> 1 : y) * pitch + i];    // libjpeg takes the plain replicating up-sampler here
    if (vs == 1) {
        const unsigned char* row = p + (long)y * pitch;
        const int near = row[i];
        if (x & 1) return i == cw - 1 ? near : (3 * near + row[i + 1] + 2) >> 2;
        return i == 0 ? near : (3 * near + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    int rn = (y & 1) ? r + 1 : r - 1;
    rn = rn < 0 ? 0 : (rn > chh - 1 ? chh - 1 : rn);
    const unsigned char* r0 = p + (long)r * pitch;
    const unsigned char* r1 = p + (long)rn * pitch;
    const int cur = 3 * r0[i] + r1[i];
    if (x & 1) return i == cw - 1 ? (cur * 4 + 7) >> 4 : (cur * 3 + (3 * r0[i + 1] + r1[i + 1]) + 7) >> 4;
    return i == 0 ? (cur * 4 + 8) >> 4 : (cur * 3 + (3 * r0[i - 1] + r1[i - 1]) + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char* __restrict__ planes, long plane_bytes, long coef_bytes,
                                                         const JpegDesc* __restrict__ desc, unsigned char* __restrict__ dst, long dst_bytes) {
    const JpegDesc& d = desc[blockIdx.z];
    const int W = d.W, H = d.H;
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= W || y >= H) return;
    const JpegGeom g = jpeg_geom(d);
    if (!jpeg_fits(d, g, coef_bytes, plane_bytes, dst_bytes)) return;
    const unsigned char* base = planes + d.plane_off;
    const int p0 = g.bw[0] * 8;
    const unsigned yw = *reinterpret_cast<const unsigned*>(base + (long)y * p0 + x0);      // x0 + 3 < p0: the plane is whole blocks wide
    unsigned char o[12];
    const int nx = W - x0 < 4 ? W - x0 : 4;
    if (d.ncomp == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[3 * k] = o[3 * k + 1] = o[3 * k + 2] = (unsigned char)((yw >> (8 * k)) & 255u);
    } else {
        const int pc = g.bw[1] * 8, cw = (W + d.hs - 1) / d.hs, chh = (H + d.vs - 1) / d.vs;
        const unsigned char* pb = base + g.start[1] * 64;
        const unsigned char* pr = base + g.start[2] * 64;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k < W ? x0 + k : W - 1;
            const int yy = (int)((yw >> (8 * k)) & 255u);
            const int cb = jpeg_chroma(pb, pc, cw, chh, d.hs, d.vs, x, y) - 128;
            const int cr = jpeg_chroma(pr, pc, cw, chh, d.hs, d.vs, x, y) - 128;
            // jdcolor.c: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 32768
            const int rr = yy + ((91881 * cr + 32768) >> 16);
            const int gg = yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
            const int bb = yy + ((116130 * cb + 32768) >> 16);
            o[3 * k] = (unsigned char)clamp255(bb);
            o[3 * k + 1] = (unsigned char)clamp255(gg);
            o[3 * k + 2] = (unsigned char)clamp255(rr);
        }
    }
    unsigned char* out = dst + d.dst_off + ((long)y * W + x0) * 3;
    if (nx == 4 && (reinterpret_cast<unsigned long long>(out) & 3ull) == 0) {
        unsigned* o4 = reinterpret_cast<unsigned*>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (unsigned)o[4 * k] | ((unsigned)o[4 * k + 1] << 8) | ((unsigned)o[4 * k + 2] << 16) | ((unsigned)o[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < nx * 3; ++k) out[k] = o[k];
    }
}

extern "C" int hn_jpeg_decode(const void* coefs, long coef_bytes, const void* desc, int N, long max_blocks, int max_h, int max_w, void* planes,
                              long plane_bytes, void* dst, long dst_bytes, hipStream_t st) {
    HN_CHECK_ARG(coefs && desc && planes && dst && N > 0 && N <= 65535 && max_blocks > 0 && max_blocks <= (1L << 30) && max_h > 0 &&
                 max_h <= 65535 && max_w > 0 && max_w <= 65535 && coef_bytes > 0 && plane_bytes > 0 && dst_bytes > 0 &&
                 ((uintptr_t)coefs & 15) == 0 && ((uintptr_t)planes & 15) == 0);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 255) / 256), (unsigned)N), dim3(256), 0, st, (const short*)coefs,
                       coef_bytes, (const JpegDesc*)desc, (unsigned char*)planes, plane_bytes, dst_bytes);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_w + 255) / 256), (unsigned)((max_h + 3) / 4), (unsigned)N), dim3(256), 0, st,
                       (const unsigned char*)planes, plane_bytes, coef_bytes, (const JpegDesc*)desc, (unsigned char*)dst, dst_bytes);
    HN_LAUNCH_CHECK();
}
