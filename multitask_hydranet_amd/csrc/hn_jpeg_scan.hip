// The JPEG decode's entropy stage on the device (jpeg.entropy_decode_device; semantics in DESIGN.md 4g, restated in Python by
// tests/jpeg_scan_ref.py): every image's entropy-coded scan, as it lies in the file, -> the quantised int16 coefficients
// hn_jpeg_entropy_decode writes, element for element.  Self-synchronising parallel Huffman decoding (Weissenberger & Schmidt): the scan is cut
// into subsequences of JPEG_SCAN_SUBSEQ raw bytes; a decoder started at a wrong bit of a Huffman stream falls into step with the right one
// after a few symbols, so every subsequence is first decoded from a guess and then again from its predecessor's exit state until no state
// changes.  A state is (bit position, block-in-MCU index m, zigzag index z); a bit position is (raw byte, bit), the reader un-stuffs FF 00 in
// line and never rests on the 00.  A subsequence owns the symbols (code + extra bits) that START in its bytes.  No workgroup waits on
// another; two memsets and three launches whatever the data:
//   jpeg_scan_sync_kernel   one workgroup per image walks the scan in windows of JPEG_SCAN_WINDOW subsequences: round 0 decodes every
//                           subsequence from (its first bit, 0, 0), later rounds those whose predecessor's exit state changed; after k
//                           rounds the first k states of the window are exact, so at most JPEG_SCAN_WINDOW rounds.  A block-count scan then
//                           gives every subsequence its first block.  Writes {entry bit, m | z << 8, first block} per subsequence; nothing else.
//   jpeg_scan_write_kernel  one thread per subsequence of every image: decodes from the exact entry state, writes AC coefficients to their
//                           de-zigzagged place in the raster-order block and the DC DIFFERENCE to entry 0; reports corrupt scans.
//   jpeg_scan_dc_kernel     one workgroup per (image, component): segmented inclusive sum of the DC differences in scan order (restarting
//                           at every restart interval), 32-bit, stored as int16.
// The state transitions depend on the bytes alone and are the same in both decoding kernels: a code that is not in the table (16 bits are
// dropped), an index past 63 and a DC category above 15 end the block; bits running out at RSTn drop the unfinished block and continue
// behind the marker with m = z = 0; at any other marker or at the end of the data the decoder stops.  Only the write kernel, whose states are
// exact, turns these into status 1, together with: an RSTn that does not follow a whole number of restart intervals (or is misnumbered, or
// has more than padding before it), a restart interval that no RSTn follows, and fewer blocks than the header's.  What follows the last
// block is ignored, as the host stage ignores it.  Every stream read is checked against the scan's length and every block against the
// image's block count.  An image whose record does not fit the buffers gets status 1 and nothing written.
#include "hn_common.h"
#include "hn_jpeg_scan.h"

#define SCAN_DONE 0xFFFFFFFFu          // the bit position of a decoder that stopped: past every subsequence

namespace {

__constant__ unsigned char c_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct ScanGeom {
    int hv, bpm;                       // luma blocks per MCU; blocks per MCU
    int bw[3];                         // blocks per row of each component plane
    long start[3];                     // first block of each plane
    long nblocks;
    long ib;                           // blocks per restart interval, 0 = none
};

__device__ __forceinline__ ScanGeom scan_geom(const JpegScanRec& r) {
    ScanGeom g;
    g.hv = r.hs * r.vs;
    g.bpm = r.ncomp == 3 ? g.hv + 2 : 1;
    g.nblocks = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = r.mcus_x * (c ? 1 : r.hs);
        g.start[c] = g.nblocks;
        if (c < r.ncomp) g.nblocks += (long)g.bw[c] * r.mcus_y * (c ? 1 : r.vs);
    }
    g.ib = (long)r.restart_interval * g.bpm;
    return g;
}

// the record's extents against the buffers handed to the entry point (uniform per image)
__device__ __forceinline__ bool scan_fits(const JpegScanRec& r, const ScanGeom& g, long stream_bytes, long coef_bytes, long nsub_max, long max_blocks) {
    if (!((r.ncomp == 1 || r.ncomp == 3) && (r.hs == 1 || r.hs == 2) && (r.vs == 1 || r.vs == 2) && r.mcus_x > 0 && r.mcus_y > 0 &&
          r.mcus_x <= 65535 && r.mcus_y <= 65535 && r.restart_interval >= 0 && r.restart_interval <= 65535))
        return false;
    if (r.ncomp == 1 && g.hv != 1) return false;
    for (int c = 0; c < r.ncomp; ++c)
        if (r.td[c] < 0 || r.td[c] > 2 || r.ta[c] < 0 || r.ta[c] > 2) return false;
    return r.scan_offset >= 0 && r.scan_bytes > 0 && r.scan_bytes < (1L << 28) && r.stream_off >= 0 && (r.stream_off & 15) == 0 &&
           ((r.stream_off + r.scan_offset + r.scan_bytes + 3) & ~3L) <= stream_bytes &&
           (r.scan_bytes + JPEG_SCAN_SUBSEQ - 1) / JPEG_SCAN_SUBSEQ <= nsub_max && g.nblocks <= max_blocks && r.coef_off >= 0 &&
           (r.coef_off & 15) == 0 && r.coef_off + g.nblocks * 128 <= coef_bytes;
}

// the tables in LDS: look[] = (length << 8) | symbol
struct ScanTab {
    unsigned short look[512];
    int maxcode[17], valoff[17];
    unsigned char vals[256];
};
struct ScanLds {
    ScanTab dc[3], ac[3];
    int td[3], ta[3];
};

__device__ __forceinline__ void load_tables(ScanLds& L, const JpegScanRec& r, int tid, int nthreads) {
    for (int t = 0; t < 6; ++t) {
        const JpegScanHuff& s = t < 3 ? r.dc[t] : r.ac[t - 3];
        ScanTab& d = t < 3 ? L.dc[t] : L.ac[t - 3];
        for (int i = tid; i < 512; i += nthreads) d.look[i] = (unsigned short)((s.look_n[i] << 8) | s.look_v[i]);
        for (int i = tid; i < 256; i += nthreads) d.vals[i] = s.vals[i];
        for (int i = tid; i < 17; i += nthreads) d.maxcode[i] = s.maxcode[i], d.valoff[i] = s.valoff[i];
    }
    if (tid < 3) L.td[tid] = r.td[tid], L.ta[tid] = r.ta[tid];
}

// MSB-first bit reader over the scan; positions are canonical: (raw byte, bit) of the next unread bit, never on a stuffed 00
struct Reader {
    const unsigned* words;             // the stream buffer as aligned words
    long base;                         // byte offset of the scan's first byte in it
    unsigned n;                        // scan bytes
    unsigned pos;                      // next raw byte to load
    unsigned long long acc;            // left aligned, `avail` real bits, zeros below
    int avail;
    unsigned ff;                       // bit k: the k-th last byte loaded was a stuffed FF (two raw bytes)
    bool stop;                         // a marker or the end of the data lies at pos
    long cw;
    unsigned w;

    __device__ __forceinline__ unsigned byte(unsigned i) {              // i < n
        const long a = base + i;
        if ((a >> 2) != cw) {
            cw = a >> 2;
            w = words[cw];
        }
        return (w >> (8 * (int)(a & 3))) & 255u;
    }
    __device__ __forceinline__ void seek(unsigned bitpos) {
        pos = bitpos >> 3;
        acc = 0;
        avail = 0;
        ff = 0;
        stop = false;
        if (bitpos & 7) {
            fill();
            take((int)(bitpos & 7));
        }
    }
    __device__ __forceinline__ void fill() {
        while (avail <= 56 && !stop) {
            if (pos >= n) { stop = true; break; }
            const unsigned b = byte(pos);
            if (b == 0xFF) {
                if (pos + 1 >= n || byte(pos + 1) != 0) { stop = true; break; }
                pos += 2;
                ff = (ff << 1) | 1u;
            } else {
                pos += 1;
                ff <<= 1;
            }
            acc |= (unsigned long long)b << (56 - avail);
            avail += 8;
        }
    }
    __device__ __forceinline__ bool take(int k) {
        if (k > avail) return false;
        acc <<= k;
        avail -= k;
        return true;
    }
    __device__ __forceinline__ unsigned bitpos() const {
        const int cnt = (avail + 7) >> 3;
        const unsigned raw = pos - (unsigned)cnt - (unsigned)__popc(ff & ((1u << cnt) - 1u));
        return raw * 8u + (unsigned)((-avail) & 7);
    }
};

#define SYM_OK 0
#define SYM_NOBITS 1
#define SYM_BAD 2

__device__ __forceinline__ int decode_sym(Reader& rd, const ScanTab& t, int& sym) {
    if (rd.avail < 16) rd.fill();
    const unsigned idx = (unsigned)(rd.acc >> 55);
    const unsigned e = t.look[idx];
    if (e >> 8) {
        sym = (int)(e & 255u);
        return rd.take((int)(e >> 8)) ? SYM_OK : SYM_NOBITS;
    }
    for (int len = 10; len <= 16; ++len) {
        const int code = (int)(rd.acc >> (64 - len));
        if (code <= t.maxcode[len]) {
            sym = t.vals[(code + t.valoff[len]) & 255];
            return rd.take(len) ? SYM_OK : SYM_NOBITS;
        }
    }
    if (rd.avail < 16) return SYM_NOBITS;
    rd.take(16);
    return SYM_BAD;
}

// sbits in 1..15
__device__ __forceinline__ bool receive_extend(Reader& rd, int sbits, int& v) {
    if (rd.avail < sbits) rd.fill();
    const int raw = (int)(rd.acc >> (64 - sbits));
    if (!rd.take(sbits)) return false;
    v = raw < (1 << (sbits - 1)) ? raw - (1 << sbits) + 1 : raw;
    return true;
}

struct ScanState {
    unsigned pos, mz;                  // bit position; m | z << 8
};

// Decodes the symbols that start in [st.pos, end_bit) from state `st`; returns the exit state and the blocks completed.  WRITE: the state is
// exact and `blk` the number of the block it is in; coefficients are written and errors reported.
template <bool WRITE>
__device__ __forceinline__ ScanState decode_subseq(Reader& rd, const ScanLds& L, const JpegScanRec& r, const ScanGeom& g, ScanState st,
                                                   unsigned end_bit, unsigned& completed, long blk, short* __restrict__ out, int* __restrict__ status) {
    completed = 0;
    if (st.pos >= end_bit) return st;
    int m = (int)(st.mz & 255u), z = (int)(st.mz >> 8);
    rd.seek(st.pos);
    bool err = false;
    long dest = -1, dest_of = -1;
    for (;;) {
        const unsigned sp = rd.bitpos();
        if (sp >= end_bit) {
            st.pos = sp;
            break;
        }
        if (WRITE) {
            if (blk >= g.nblocks) {                                      // what follows the last block is ignored
                st.pos = SCAN_DONE;
                break;
            }
            if (dest_of != blk) {
                const long mcu = blk / g.bpm;
                const int mm = (int)(blk - mcu * g.bpm);
                const int my = (int)(mcu / r.mcus_x), mx = (int)(mcu - (long)my * r.mcus_x);
                const int c = mm < g.hv ? 0 : mm - g.hv + 1;
                const int v = c ? 0 : mm / r.hs, u = c ? 0 : mm - v * r.hs;
                dest = g.start[c] + ((long)my * (c ? 1 : r.vs) + v) * g.bw[c] + (long)mx * (c ? 1 : r.hs) + u;
                dest_of = blk;
            }
        }
        const int comp = m < g.hv ? 0 : m - g.hv + 1;
        bool block_end = false, nobits = false;
        if (z == 0) {
            int s;
            const int rc = decode_sym(rd, L.dc[L.td[comp]], s);
            if (rc == SYM_NOBITS) {
                nobits = true;
            } else if (rc == SYM_BAD || s > 15) {
                err = true;
                block_end = true;
            } else {
                int diff = 0;
                if (s && !receive_extend(rd, s, diff)) {
                    nobits = true;
                } else {
                    if (WRITE) out[dest * 64] = (short)diff;
                    z = 1;
                }
            }
        } else {
            int rs;
            const int rc = decode_sym(rd, L.ac[L.ta[comp]], rs);
            if (rc == SYM_NOBITS) {
                nobits = true;
            } else if (rc == SYM_BAD) {
                err = true;
                block_end = true;
            } else {
                const int run = rs >> 4, sz = rs & 15;
                if (sz) {
                    const int k = z + run;
                    int v;
                    if (k > 63) {
                        err = true;
                        block_end = true;
                    } else if (!receive_extend(rd, sz, v)) {
                        nobits = true;
                    } else {
                        if (WRITE) out[dest * 64 + c_natural[k]] = (short)v;
                        z = k + 1;
                        block_end = z > 63;
                    }
                } else if (run == 15) {
                    z += 16;
                    block_end = z > 63;
                } else {
                    block_end = true;
                }
            }
        }
        if (nobits) {
            // the reader rests on a marker or on the end of the data: RSTn drops the unfinished block, anything else ends the decode
            unsigned i = rd.pos;
            while (i + 1 < rd.n && rd.byte(i) == 0xFF && rd.byte(i + 1) == 0xFF) ++i;
            const unsigned mk = i + 1 < rd.n && rd.byte(i) == 0xFF ? rd.byte(i + 1) : 0u;
            if (mk < 0xD0 || mk > 0xD7) {
                err = true;
                st.pos = SCAN_DONE;
                break;
            }
            if (WRITE) {
                // exact: only padding may be dropped, after a whole number of restart intervals, before the marker of that number
                const long iv = g.ib ? blk / g.ib : 0;
                if (!(g.ib && z == 0 && m == 0 && rd.avail < 8 && blk > 0 && iv * g.ib == blk && ((iv - 1) & 7) == (long)(mk - 0xD0))) err = true;
            }
            m = 0;
            z = 0;
            rd.seek((i + 2) * 8u);
            continue;
        }
        if (block_end) {
            ++completed;
            m = m + 1 == g.bpm ? 0 : m + 1;
            z = 0;
            if (WRITE) {
                ++blk;
                if (g.ib && blk < g.nblocks && blk % g.ib == 0) {        // a restart interval is complete: RSTn follows the padding
                    const unsigned bp = rd.bitpos();
                    unsigned i = bp >> 3;
                    if (bp & 7) i += rd.byte(i) == 0xFF ? 2 : 1;
                    while (i + 1 < rd.n && rd.byte(i) == 0xFF && rd.byte(i + 1) == 0xFF) ++i;
                    if (!(i + 1 < rd.n && rd.byte(i) == 0xFF && (rd.byte(i + 1) & 0xF8) == 0xD0)) err = true;
                }
            }
        }
    }
    st.mz = (unsigned)m | ((unsigned)z << 8);
    if (WRITE && err) atomicOr(status, 1);
    return st;
}

__device__ __forceinline__ Reader make_reader(const void* streams, const JpegScanRec& r) {
    Reader rd;
    rd.words = (const unsigned*)streams;
    rd.base = r.stream_off + r.scan_offset;
    rd.n = (unsigned)r.scan_bytes;
    rd.cw = -1;
    rd.w = 0;
    rd.pos = 0, rd.acc = 0, rd.avail = 0, rd.ff = 0, rd.stop = false;
    return rd;
}

__global__ __launch_bounds__(JPEG_SCAN_WINDOW) void jpeg_scan_sync_kernel(const void* __restrict__ streams, long stream_bytes,
                                                                          const JpegScanRec* __restrict__ recs, uint4* __restrict__ ws,
                                                                          long nsub_max, long max_blocks, long coef_bytes, int* __restrict__ status) {
    constexpr int T = JPEG_SCAN_WINDOW;
    __shared__ ScanLds L;
    __shared__ unsigned ex_pos[T + 1], ex_mz[T + 1];                    // [t + 1]: exit state of thread t; [0]: the window's exact entry
    __shared__ unsigned cnt[T];
    const int img = blockIdx.x, tid = threadIdx.x;
    const JpegScanRec& r = recs[img];
    const ScanGeom g = scan_geom(r);
    if (!scan_fits(r, g, stream_bytes, coef_bytes, nsub_max, max_blocks)) {
        if (tid == 0) atomicOr(status + img, 1);
        return;
    }
    load_tables(L, r, tid, T);
    if (tid == 0) ex_pos[0] = 0, ex_mz[0] = 0;
    __syncthreads();
    Reader rd = make_reader(streams, r);
    const unsigned n = rd.n;
    const long nsub = ((long)n + JPEG_SCAN_SUBSEQ - 1) / JPEG_SCAN_SUBSEQ;
    unsigned blockbase = 0;
    for (long w0 = 0; w0 < nsub; w0 += T) {
        const long i = w0 + tid;
        const bool active = i < nsub;
        const unsigned end_bit = active ? (unsigned)((i + 1) * JPEG_SCAN_SUBSEQ < (long)n ? (i + 1) * JPEG_SCAN_SUBSEQ : (long)n) * 8u : 0u;
        ScanState in = {ex_pos[0], ex_mz[0]};
        if (tid != 0 && active) {
            unsigned b = (unsigned)(i * JPEG_SCAN_SUBSEQ);
            if (rd.byte(b - 1) == 0xFF) ++b;                            // not on a stuffed 00, not inside a marker
            in.pos = b * 8u;
            in.mz = 0;
        }
        unsigned c = 0;
        ScanState outst = in;
        if (active) outst = decode_subseq<false>(rd, L, r, g, in, end_bit, c, 0, nullptr, nullptr);
        __syncthreads();                                                 // ex[0] read by everyone
        ex_pos[tid + 1] = outst.pos, ex_mz[tid + 1] = outst.mz;
        cnt[tid] = c;
        __syncthreads();
        for (int round = 1; round <= T; ++round) {
            const ScanState nin = {ex_pos[tid], ex_mz[tid]};
            const bool changed = active && (nin.pos != in.pos || nin.mz != in.mz);
            __syncthreads();
            if (changed) {
                in = nin;
                outst = decode_subseq<false>(rd, L, r, g, in, end_bit, c, 0, nullptr, nullptr);
                ex_pos[tid + 1] = outst.pos, ex_mz[tid + 1] = outst.mz;
                cnt[tid] = c;
            }
            if (!__syncthreads_or(changed ? 1 : 0)) break;
        }
        // inclusive scan of the block counts
        for (int d = 1; d < T; d <<= 1) {
            const unsigned add = tid >= d ? cnt[tid - d] : 0u;
            __syncthreads();
            cnt[tid] += add;
            __syncthreads();
        }
        if (active) ws[(long)img * nsub_max + i] = make_uint4(in.pos, in.mz, blockbase + cnt[tid] - c, 0u);
        blockbase += cnt[T - 1];
        const int last = (int)(nsub - w0 < T ? nsub - w0 : T);
        const unsigned cp = ex_pos[last], cm = ex_mz[last];
        __syncthreads();
        if (tid == 0) ex_pos[0] = cp, ex_mz[0] = cm;
        __syncthreads();
    }
    if (tid == 0 && (long)blockbase < g.nblocks) atomicOr(status + img, 1);
}

__global__ __launch_bounds__(256) void jpeg_scan_write_kernel(const void* __restrict__ streams, long stream_bytes,
                                                              const JpegScanRec* __restrict__ recs, const uint4* __restrict__ ws, long nsub_max,
                                                              long max_blocks, short* __restrict__ coefs, long coef_bytes, int* __restrict__ status) {
    __shared__ ScanLds L;
    const int img = blockIdx.y, tid = threadIdx.x;
    const JpegScanRec& r = recs[img];
    const ScanGeom g = scan_geom(r);
    if (!scan_fits(r, g, stream_bytes, coef_bytes, nsub_max, max_blocks)) return;
    const long nsub = (r.scan_bytes + JPEG_SCAN_SUBSEQ - 1) / JPEG_SCAN_SUBSEQ;
    if ((long)blockIdx.x * 256 >= nsub) return;
    load_tables(L, r, tid, 256);
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + tid;
    if (i >= nsub) return;
    Reader rd = make_reader(streams, r);
    const uint4 e = ws[(long)img * nsub_max + i];
    const long end = (i + 1) * JPEG_SCAN_SUBSEQ < r.scan_bytes ? (i + 1) * JPEG_SCAN_SUBSEQ : r.scan_bytes;
    unsigned c;
    decode_subseq<true>(rd, L, r, g, ScanState{e.x, e.y}, (unsigned)end * 8u, c, (long)e.z, coefs + (r.coef_off >> 1), status + img);
}

// segmented sum: (flag, value) pairs, a set flag cuts off what lies to the left
__global__ __launch_bounds__(256) void jpeg_scan_dc_kernel(long stream_bytes, const JpegScanRec* __restrict__ recs, long nsub_max, long max_blocks,
                                                           short* __restrict__ coefs, long coef_bytes) {
    __shared__ int s_sum[256];
    __shared__ int s_flag[256];
    const int img = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const JpegScanRec& r = recs[img];
    const ScanGeom g = scan_geom(r);
    if (c >= r.ncomp || !scan_fits(r, g, stream_bytes, coef_bytes, nsub_max, max_blocks)) return;
    const int per = c ? 1 : g.hv, ch = c ? 1 : r.hs, cv = c ? 1 : r.vs;
    const long count = (long)r.mcus_x * r.mcus_y * per;
    const long seg = r.restart_interval ? (long)r.restart_interval * per : count;
    const long len = (count + 255) / 256;
    const long j0 = tid * len, j1 = j0 + len < count ? j0 + len : count;
    short* base = coefs + (r.coef_off >> 1);
    auto place = [&](long j) {
        const long mcu = j / per;
        const int q = (int)(j - mcu * per);
        const int v = q / ch, u = q - v * ch;
        const int my = (int)(mcu / r.mcus_x), mx = (int)(mcu - (long)my * r.mcus_x);
        return (g.start[c] + ((long)my * cv + v) * g.bw[c] + (long)mx * ch + u) * 64;
    };
    int sum = 0, flag = 0;
    for (long j = j0; j < j1; ++j) {
        if (j % seg == 0) sum = 0, flag = 1;
        sum += base[place(j)];
    }
    s_sum[tid] = sum, s_flag[tid] = flag;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        int a = 0, f = 0;
        if (tid >= d) a = s_sum[tid - d], f = s_flag[tid - d];
        __syncthreads();
        if (tid >= d) {
            if (!s_flag[tid]) s_sum[tid] += a;
            s_flag[tid] |= f;
        }
        __syncthreads();
    }
    int pred = tid ? s_sum[tid - 1] : 0;
    for (long j = j0; j < j1; ++j) {
        if (j % seg == 0) pred = 0;
        const long o = place(j);
        pred += base[o];
        base[o] = (short)pred;
    }
}

}  // namespace

extern "C" int hn_jpeg_scan_subseq_bytes(void) { return JPEG_SCAN_SUBSEQ; }

extern "C" long hn_jpeg_scan_ws_bytes(int N, long max_scan_bytes, long max_blocks) {
    if (N <= 0 || max_scan_bytes <= 0 || max_scan_bytes >= (1L << 28) || max_blocks <= 0) return -1;
    return (long)N * ((max_scan_bytes + JPEG_SCAN_SUBSEQ - 1) / JPEG_SCAN_SUBSEQ) * 16;
}

extern "C" int hn_jpeg_scan_decode(const void* streams, long stream_bytes, const void* desc, int N, long max_scan_bytes, long max_blocks,
                                   void* ws, long ws_bytes, void* coefs, long coef_bytes, void* status, hipStream_t st) {
    HN_CHECK_ARG(streams && desc && ws && coefs && status && N > 0 && N <= 65535 && max_scan_bytes > 0 && max_scan_bytes < (1L << 28) &&
                 max_blocks > 0 && max_blocks <= (1L << 30) && stream_bytes > 0 && (stream_bytes & 3) == 0 && coef_bytes > 0 &&
                 ((uintptr_t)streams & 15) == 0 && ((uintptr_t)coefs & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)desc & 7) == 0 &&
                 ws_bytes >= hn_jpeg_scan_ws_bytes(N, max_scan_bytes, max_blocks));
    const long nsub_max = (max_scan_bytes + JPEG_SCAN_SUBSEQ - 1) / JPEG_SCAN_SUBSEQ;
    const JpegScanRec* recs = (const JpegScanRec*)desc;
    if (hipMemsetAsync(status, 0, (size_t)N * 4, st) != hipSuccess) return HN_ERR_LAUNCH;
    if (hipMemsetAsync(coefs, 0, (size_t)coef_bytes, st) != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_scan_sync_kernel, dim3((unsigned)N), dim3(JPEG_SCAN_WINDOW), 0, st, streams, stream_bytes, recs, (uint4*)ws, nsub_max,
                       max_blocks, coef_bytes, (int*)status);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_scan_write_kernel, dim3((unsigned)((nsub_max + 255) / 256), (unsigned)N), dim3(256), 0, st, streams, stream_bytes,
                       recs, (const uint4*)ws, nsub_max, max_blocks, (short*)coefs, coef_bytes, (int*)status);
    if (hipGetLastError() != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_scan_dc_kernel, dim3(3, (unsigned)N), dim3(256), 0, st, stream_bytes, recs, nsub_max, max_blocks, (short*)coefs,
                       coef_bytes);
    HN_LAUNCH_CHECK();
}
