// Training-batch assembly and augmentation on the device (augment.py; semantics in its module docstring and DESIGN.md 4f, restated in
// float64 numpy by tests/augment_ref.py).  The host samples one plan per image and hands a ragged batch of uint8 BGR source frames (one
// packed buffer, per-image byte offsets) with one AugDesc per image; every per-pixel step runs here:
//
//   aug_photo_kernel  the photometric op at source resolution, only for images that have one (ws_off >= 0), into the workspace:
//                     separable Gaussian blur (LDS tile, fp32 horizontal then vertical pass, reflect-101 border), linear contrast,
//                     multiply, additive Gaussian noise (Philox4x32-10 + Box-Muller), HSV channel multiply (OpenCV's 8-bit RGB<->HSV).
//   aug_image_kernel  one thread per network-size output pixel: the INTER_AREA footprint of the pixel over the (never stored) warped
//                     intermediate frame, each intermediate pixel = round(bilinear sample at F^-1(centre)), zero fill outside; then
//                     BGR -> RGB and (v/255 - mean)/std in double, fp32 NCHW (exactly as hn_preprocess_bgr does).
//   aug_seg_kernel    one thread per network-size label: INTER_NEAREST index into the intermediate frame, its centre through F^-1, floor.
//
// Every rounding is explicit (rint = round half to even, as cvRound) and FMA contraction is off for the whole file, so the fp32 / fp64
// expressions evaluate exactly as the numpy restatement writes them.
#include "hn_common.h"

#pragma clang fp contract(off)

// per-image descriptor, mirrored by augment.py DESC_DTYPE (176 bytes)
struct AugDesc {
    double finv[6];            // augmented-frame -> source: xs = f0*x + f1*y + f2, ys = f3*x + f4*y + f5
    double p[4];               // op parameters: contrast alpha | multiply f0..f2 | noise scale | HSV factor
    long src_off;              // byte offset of the BGR frame in src
    long ws_off;               // byte offset of its photometric output in ws, -1 = no photometric op (sample src)
    long seg_off;              // byte offset of the label map in seg, -1 = none
    int Hs, Ws;
    int op, per_channel;       // AUG_OP_*; noise / multiply: one value per channel
    unsigned seed_lo, seed_hi; // Philox key of the noise
    int radius, pad0;          // blur radius (<= AUG_MAX_R)
    float w[8];                // blur weights w[0..radius] (symmetric)
    long pad1;
};
static_assert(sizeof(AugDesc) == 176, "AugDesc layout is mirrored by augment.py");

#define AUG_OP_NONE 0
#define AUG_OP_BLUR 1
#define AUG_OP_CONTRAST 2
#define AUG_OP_MULTIPLY 3
#define AUG_OP_NOISE 4
#define AUG_OP_HUE 5
#define AUG_OP_SAT 6
#define AUG_OP_VAL 7
#define AUG_MAX_R 7

// photometric tile: 64 x 16 pixels, 256 threads
#define PT_W 64
#define PT_H 16

__device__ __forceinline__ int clamp_u8(double v) { return v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v); }
__device__ __forceinline__ int clamp_u8f(float v) { return v < 0.f ? 0 : (v > 255.f ? 255 : (int)v); }

__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// OpenCV's 8-bit RGB -> HSV (hsv_shift 12, H in [0, 180)), the selected channel times f (H wraps mod 180, S / V clamp), fp32 HSV -> RGB
__device__ void hsv_mul(int& r, int& g, int& b, int ch, double f) {
    int v = r > g ? r : g;
    v = v > b ? v : b;
    int vmin = r < g ? r : g;
    vmin = vmin < b ? vmin : b;
    const int diff = v - vmin;
    const int sdiv = v ? (int)rint((double)(255 << 12) / (double)v) : 0;
    const int hdiv = diff ? (int)rint((double)(180 << 12) / (6.0 * diff)) : 0;
    int s = (diff * sdiv + (1 << 11)) >> 12;
    int h = v == r ? (g - b) : (v == g ? (b - r + 2 * diff) : (r - g + 4 * diff));
    h = (h * hdiv + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    if (ch == 0) {
        h = (int)rint((double)h * f) % 180;
    } else if (ch == 1) {
        s = clamp_u8(rint((double)s * f));
    } else {
        v = clamp_u8(rint((double)v * f));
    }
    const float hf = (float)h, sf = (float)s * (1.f / 255.f), vf = (float)v * (1.f / 255.f);
    float ro, go, bo;
    if (sf == 0.f) {
        ro = go = bo = vf;
    } else {
        float hh = hf * (6.f / 180.f);
        while (hh < 0.f) hh += 6.f;
        while (hh >= 6.f) hh -= 6.f;
        int sector = (int)floorf(hh);
        hh -= (float)sector;
        if (sector < 0 || sector >= 6) { sector = 0; hh = 0.f; }
        float tab[4];
        tab[0] = vf;
        tab[1] = vf * (1.f - sf);
        tab[2] = vf * (1.f - sf * hh);
        tab[3] = vf * (1.f - sf * (1.f - hh));
        // OpenCV's sector_data, (b, g, r) tab indices per sector
        const int sb[6] = {1, 1, 3, 0, 0, 2}, sg[6] = {3, 0, 0, 2, 1, 1}, sr[6] = {0, 2, 1, 1, 3, 0};
        bo = tab[sb[sector]]; go = tab[sg[sector]]; ro = tab[sr[sector]];
    }
    r = clamp_u8f(rintf(ro * 255.f));
    g = clamp_u8f(rintf(go * 255.f));
    b = clamp_u8f(rintf(bo * 255.f));
}

__global__ __launch_bounds__(256) void aug_photo_kernel(const unsigned char* __restrict__ src, const AugDesc* __restrict__ desc,
                                                        unsigned char* __restrict__ ws) {
    const AugDesc& d = desc[blockIdx.z];
    const int op = d.op, Hs = d.Hs, Ws = d.Ws;
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    if (op == AUG_OP_NONE || d.ws_off < 0 || x0 >= Ws || y0 >= Hs) return;
    const unsigned char* im = src + d.src_off;
    unsigned char* out = ws + d.ws_off;
    const int tx = threadIdx.x % PT_W, ty = threadIdx.x / PT_W;         // 64 x 4
    if (op == AUG_OP_BLUR) {
        __shared__ unsigned char s_in[PT_H + 2 * AUG_MAX_R][(PT_W + 2 * AUG_MAX_R) * 3];
        __shared__ float s_h[PT_H + 2 * AUG_MAX_R][PT_W * 3];
        const int R = d.radius;
        const int rows = PT_H + 2 * R, cols = PT_W + 2 * R;
        for (int i = threadIdx.x; i < rows * cols * 3; i += 256) {
            const int rr = i / (cols * 3), q = i - rr * cols * 3, cc = q / 3, ch = q - cc * 3;
            int ys = y0 - R + rr, xs = x0 - R + cc;                      // reflect-101
            ys = ys < 0 ? -ys : (ys >= Hs ? 2 * Hs - 2 - ys : ys);
            xs = xs < 0 ? -xs : (xs >= Ws ? 2 * Ws - 2 - xs : xs);
            ys = ys < 0 ? 0 : (ys >= Hs ? Hs - 1 : ys);                  // (frames narrower than the kernel)
            xs = xs < 0 ? 0 : (xs >= Ws ? Ws - 1 : xs);
            s_in[rr][cc * 3 + ch] = im[((long)ys * Ws + xs) * 3 + ch];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < rows * PT_W * 3; i += 256) {
            const int rr = i / (PT_W * 3), q = i - rr * PT_W * 3, cc = q / 3, ch = q - cc * 3;
            float acc = 0.f;
            for (int k = -R; k <= R; ++k) acc = acc + d.w[k < 0 ? -k : k] * (float)s_in[rr][(cc + R + k) * 3 + ch];
            s_h[rr][cc * 3 + ch] = acc;
        }
        __syncthreads();
        const int x = x0 + tx;
        if (x >= Ws) return;
        for (int r = ty; r < PT_H; r += 4) {
            const int y = y0 + r;
            if (y >= Hs) break;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float acc = 0.f;
                for (int k = -R; k <= R; ++k) acc = acc + d.w[k < 0 ? -k : k] * s_h[r + R + k][tx * 3 + ch];
                out[((long)y * Ws + x) * 3 + ch] = (unsigned char)clamp_u8f(rintf(acc));
            }
        }
        return;
    }
    const int x = x0 + tx;
    if (x >= Ws) return;
    for (int r = ty; r < PT_H; r += 4) {
        const int y = y0 + r;
        if (y >= Hs) break;
        const long pix = (long)y * Ws + x;
        const unsigned char* p = im + pix * 3;
        int c[3] = {p[0], p[1], p[2]};
        if (op == AUG_OP_CONTRAST) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = clamp_u8(rint(127.5 + d.p[0] * ((double)c[ch] - 127.5)));
        } else if (op == AUG_OP_MULTIPLY) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = clamp_u8(rint((double)c[ch] * d.p[ch]));
        } else if (op == AUG_OP_NOISE) {
            unsigned ctr[4] = {(unsigned)pix, (unsigned)(pix >> 32), 0u, 0u};
            philox4x32_10(ctr, d.seed_lo, d.seed_hi);
            const double two32 = 4294967296.0, two_pi = 6.283185307179586;
            const double r0 = sqrt(-2.0 * log(((double)ctr[0] + 1.0) / two32));
            const double r1 = sqrt(-2.0 * log(((double)ctr[2] + 1.0) / two32));
            const double z[3] = {r0 * cos(two_pi * ((double)ctr[1] / two32)), r0 * sin(two_pi * ((double)ctr[1] / two32)),
                                 r1 * cos(two_pi * ((double)ctr[3] / two32))};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = clamp_u8(rint((double)c[ch] + d.p[0] * z[d.per_channel ? ch : 0]));
        } else {
            hsv_mul(c[0], c[1], c[2], op - AUG_OP_HUE, d.p[0]);     // the buffer's bytes read as (R, G, B), as the reference hands them over
        }
        unsigned char* o = out + pix * 3;
        o[0] = (unsigned char)c[0]; o[1] = (unsigned char)c[1]; o[2] = (unsigned char)c[2];
    }
}

// one intermediate (warped, source-size) pixel: bilinear in pixel-centre space at F^-1(sx + 0.5, sy + 0.5), zero fill, rounded
__device__ __forceinline__ void warp_px(const unsigned char* im, int Hs, int Ws, const double* F, int sx, int sy, float v[3]) {
    const double cx = (double)sx + 0.5, cy = (double)sy + 0.5;
    const double u = (F[0] * cx + F[1] * cy + F[2]) - 0.5;
    const double w = (F[3] * cx + F[4] * cy + F[5]) - 0.5;
    v[0] = v[1] = v[2] = 0.f;
    if (!(u > -1.0 && w > -1.0 && u < (double)Ws && w < (double)Hs)) return;   // every tap outside (NaN included)
    const double fu = floor(u), fw = floor(w);
    const int x0 = (int)fu, y0 = (int)fw;
    const double ax = u - fu, ay = w - fw;
    if (ax == 0.0 && ay == 0.0) {                                    // on a source pixel centre: the sample is that pixel
        if (x0 >= 0 && y0 >= 0) {
            const unsigned char* p = im + ((long)y0 * Ws + x0) * 3;
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        }
        return;
    }
    const bool xa = x0 >= 0, xb = x0 + 1 < Ws, ya = y0 >= 0, yb = y0 + 1 < Hs;
    const unsigned char* r0 = im + (long)y0 * Ws * 3;
    const unsigned char* r1 = r0 + (long)Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p00 = (ya && xa) ? (double)r0[x0 * 3 + c] : 0.0;
        const double p01 = (ya && xb) ? (double)r0[(x0 + 1) * 3 + c] : 0.0;
        const double p10 = (yb && xa) ? (double)r1[x0 * 3 + c] : 0.0;
        const double p11 = (yb && xb) ? (double)r1[(x0 + 1) * 3 + c] : 0.0;
        const double val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11);
        v[c] = (float)clamp_u8(rint(val));
    }
}

// cv::resize INTER_AREA taps of output coordinate dc along one axis (computeResizeAreaTab): the source indices are contiguous,
// [first, first + n); a partial head, full-cell middle taps, a partial tail
struct AreaAxis {
    int first, n, head, tail;
    float a_head, a_mid, a_tail;
    __device__ __forceinline__ float alpha(int k) const { return (k == 0 && head) ? a_head : ((k == n - 1 && tail) ? a_tail : a_mid); }
};

__device__ __forceinline__ AreaAxis area_axis(int dc, double scale, int ssize) {
    const double f1 = (double)dc * scale, f2 = f1 + scale;
    const double cell = scale < (double)ssize - f1 ? scale : (double)ssize - f1;
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = s2 < ssize - 1 ? s2 : ssize - 1;
    s1 = s1 < s2 ? s1 : s2;
    AreaAxis a;
    a.head = (double)s1 - f1 > 1e-3;
    a.tail = f2 - (double)s2 > 1e-3;
    a.first = a.head ? s1 - 1 : s1;
    a.n = a.head + (s2 - s1) + a.tail;
    a.a_head = (float)(((double)s1 - f1) / cell);
    a.a_mid = (float)(1.0 / cell);
    double t = f2 - (double)s2;
    t = t < 1.0 ? t : 1.0;
    t = t < cell ? t : cell;
    a.a_tail = (float)(t / cell);
    return a;
}


__global__ __launch_bounds__(256) void aug_image_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ ws,
                                                        const AugDesc* __restrict__ desc, int Hd, int Wd, float* __restrict__ dst) {
    const int x = blockIdx.x * 64 + threadIdx.x % 64, y = blockIdx.y * 4 + threadIdx.x / 64, n = blockIdx.z;
    if (x >= Wd || y >= Hd) return;
    const AugDesc& d = desc[n];
    const int Hs = d.Hs, Ws = d.Ws;
    const unsigned char* im = d.ws_off >= 0 ? ws + d.ws_off : src + d.src_off;
    double F[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) F[i] = d.finv[i];
    const double sx_ = 1.0 / ((double)Wd / (double)Ws), sy_ = 1.0 / ((double)Hd / (double)Hs);
    const double isx = rint(sx_), isy = rint(sy_);
    float acc[3];
    if (fabs(sx_ - isx) < 2.220446049250313e-16 && fabs(sy_ - isy) < 2.220446049250313e-16) {
        // resizeAreaFast: the integer block sum times 1/area
        const int kx = (int)isx, ky = (int)isy;
        int sum[3] = {0, 0, 0};
        for (int j = 0; j < ky; ++j)
            for (int i = 0; i < kx; ++i) {
                float v[3];
                warp_px(im, Hs, Ws, F, x * kx + i, y * ky + j, v);
                sum[0] += (int)v[0]; sum[1] += (int)v[1]; sum[2] += (int)v[2];
            }
        const float sc = 1.f / (float)(kx * ky);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = (float)sum[c] * sc;
    } else {
        // resizeArea: per source row the alpha-weighted row sum (fp32, tap order), then the beta-weighted sum over rows
        const AreaAxis ax = area_axis(x, sx_, Ws), ay = area_axis(y, sy_, Hs);
        acc[0] = acc[1] = acc[2] = 0.f;
        for (int j = 0; j < ay.n; ++j) {
            float buf[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < ax.n; ++i) {
                float v[3];
                warp_px(im, Hs, Ws, F, ax.first + i, ay.first + j, v);
                const float a = ax.alpha(i);
#pragma unroll
                for (int c = 0; c < 3; ++c) buf[c] = buf[c] + v[c] * a;
            }
            const float b = ay.alpha(j);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + b * buf[c];
        }
    }
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    const long plane = (long)Hd * Wd;
    float* o = dst + (long)n * 3 * plane + (long)y * Wd + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                   // output channel c = R, G, B = intermediate channel 2 - c (BGR)
        const int v = clamp_u8f(rintf(acc[2 - c]));
        o[c * plane] = (float)(((double)v / 255.0 - mean[c]) / sd[c]);
    }
}

__global__ __launch_bounds__(256) void aug_seg_kernel(const unsigned char* __restrict__ seg, const AugDesc* __restrict__ desc, int Hd, int Wd,
                                                      unsigned char* __restrict__ dst) {
    const int x = blockIdx.x * 64 + threadIdx.x % 64, y = blockIdx.y * 4 + threadIdx.x / 64, n = blockIdx.z;
    if (x >= Wd || y >= Hd) return;
    const AugDesc& d = desc[n];
    const int Hs = d.Hs, Ws = d.Ws;
    int ix = (int)floor((double)x * (1.0 / ((double)Wd / (double)Ws)));
    int iy = (int)floor((double)y * (1.0 / ((double)Hd / (double)Hs)));
    ix = ix < Ws - 1 ? ix : Ws - 1;
    iy = iy < Hs - 1 ? iy : Hs - 1;
    const double cx = (double)ix + 0.5, cy = (double)iy + 0.5;
    const double u = floor(d.finv[0] * cx + d.finv[1] * cy + d.finv[2]);
    const double w = floor(d.finv[3] * cx + d.finv[4] * cy + d.finv[5]);
    unsigned char v = 0;
    if (d.seg_off >= 0 && u >= 0.0 && w >= 0.0 && u < (double)Ws && w < (double)Hs) v = seg[d.seg_off + (long)w * Ws + (long)u];
    dst[(long)n * Hd * Wd + (long)y * Wd + x] = v;
}

extern "C" int hn_augment_photometric(const void* src, const void* desc, int N, int max_hs, int max_ws, void* ws, hipStream_t st) {
    HN_CHECK_ARG(src && desc && ws && N > 0 && N <= 65535 && max_hs > 0 && max_ws > 0);
    const dim3 grid((unsigned)((max_ws + PT_W - 1) / PT_W), (unsigned)((max_hs + PT_H - 1) / PT_H), (unsigned)N);
    hipLaunchKernelGGL(aug_photo_kernel, grid, dim3(256), 0, st, (const unsigned char*)src, (const AugDesc*)desc, (unsigned char*)ws);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_augment_image(const void* src, const void* ws, const void* desc, int N, int Hd, int Wd, float* dst, hipStream_t st) {
    HN_CHECK_ARG(src && desc && dst && N > 0 && N <= 65535 && Hd > 0 && Wd > 0);
    const dim3 grid((unsigned)((Wd + 63) / 64), (unsigned)((Hd + 3) / 4), (unsigned)N);
    hipLaunchKernelGGL(aug_image_kernel, grid, dim3(256), 0, st, (const unsigned char*)src, (const unsigned char*)ws, (const AugDesc*)desc,
                       Hd, Wd, dst);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_augment_seg(const void* seg, const void* desc, int N, int Hd, int Wd, void* dst, hipStream_t st) {
    HN_CHECK_ARG(seg && desc && dst && N > 0 && N <= 65535 && Hd > 0 && Wd > 0);
    const dim3 grid((unsigned)((Wd + 63) / 64), (unsigned)((Hd + 3) / 4), (unsigned)N);
    hipLaunchKernelGGL(aug_seg_kernel, grid, dim3(256), 0, st, (const unsigned char*)seg, (const AugDesc*)desc, Hd, Wd, (unsigned char*)dst);
    HN_LAUNCH_CHECK();
}
