// Drawing on packed BGR frames (draw.py; semantics in DESIGN.md 4h, restated in numpy by tests/draw_ref.py): one launch paints a ragged
// batch in place from a flat, ORDERED list of primitives per image.  A pixel takes the colour of the last primitive of its image's list
// that covers it, whatever the scheduling: every pixel walks the list in order and is written once, by its own thread.
//   kind 0  thick segment (x0, y0) - (x1, y1), thickness `param`: the pixel centres within param / 2 of the segment -- the distance test
//           lane_raster_kernel (hn_post.hip) uses for cv2.line, the project's one restatement of OpenCV's thick line
//   kind 1  filled rectangle, both corners inclusive, in any order
//   kind 2  glyph: a 5 x 7 bitmap (rows 0..3 in x1, rows 4..6 in y1, 5 bits per row, the left column in the high bit), every bit a
//           `param` x `param` square, top-left corner at (x0, y0)
// One workgroup per 64 x 32 pixel tile: the primitives are culled against the tile by their bounding boxes, 256 at a time, into an ordered
// LDS list (wave ballots keep the order), and only the survivors reach the per-pixel tests.  Untouched pixels are neither read nor written.
#include "hn_common.h"

struct DrawPrim {                      // draw.py PRIM_DTYPE (32 bytes)
    int kind, x0, y0, x1, y1, param;
    unsigned color;                    // b | g << 8 | r << 16
    int pad;
};
static_assert(sizeof(DrawPrim) == 32, "DrawPrim layout is mirrored by draw.py");

struct DrawImage {                     // draw.py IMAGE_DTYPE (24 bytes)
    long off;                          // byte offset of the H x W x 3 frame
    int W, H;
    int p0, p1;                        // its primitives: [p0, p1) of the list
};
static_assert(sizeof(DrawImage) == 24, "DrawImage layout is mirrored by draw.py");

#define DRAW_TW 64
#define DRAW_TH 32

__device__ __forceinline__ int draw_reach(int t) { return (2 * t + 3) / 4 + 1; }     // lane_raster_kernel's radius for width2 = 2 t

__device__ __forceinline__ bool draw_covers(const DrawPrim& p, int x, int y) {
    if (p.kind == 0) {
        const long dx = p.x1 - p.x0, dy = p.y1 - p.y0, len2 = dx * dx + dy * dy;
        const long px = x - p.x0, py = y - p.y0;
        const long dot = px * dx + py * dy;
        long num, den;                                                   // distance^2 = num / den
        if (len2 == 0 || dot <= 0) { num = px * px + py * py; den = 1; }
        else if (dot >= len2) { const long qx = x - p.x1, qy = y - p.y1; num = qx * qx + qy * qy; den = 1; }
        else { const long cr = px * dy - py * dx; num = cr * cr; den = len2; }
        return num <= (((long)p.param * p.param * den) >> 2);            // 4 distance^2 <= thickness^2 (coordinates are within +-2^14)
    }
    if (p.kind == 1) return x >= min(p.x0, p.x1) && x <= max(p.x0, p.x1) && y >= min(p.y0, p.y1) && y <= max(p.y0, p.y1);
    const int lx = x - p.x0, ly = y - p.y0;
    if (lx < 0 || ly < 0 || lx >= 5 * p.param || ly >= 7 * p.param) return false;
    const int cx = lx / p.param, cy = ly / p.param;
    const unsigned rows = cy < 4 ? (unsigned)p.x1 >> (5 * cy) : (unsigned)p.y1 >> (5 * (cy - 4));
    return (rows >> (4 - cx)) & 1u;
}

__global__ __launch_bounds__(256) void draw_kernel(unsigned char* __restrict__ frames, long frames_bytes, const DrawImage* __restrict__ imgs,
                                                   const DrawPrim* __restrict__ prims, int nprims) {
    __shared__ DrawPrim s_p[256];
    __shared__ int s_cnt[4];
    const DrawImage im = imgs[blockIdx.z];
    const int tx0 = blockIdx.x * DRAW_TW, ty0 = blockIdx.y * DRAW_TH;
    if (im.W <= 0 || im.H <= 0 || im.W > 16384 || im.H > 16384 || tx0 >= im.W || ty0 >= im.H) return;
    if (im.off < 0 || im.off + (long)im.H * im.W * 3 > frames_bytes || im.p0 < 0 || im.p1 < im.p0 || im.p1 > nprims) return;
    const int tx1 = min(tx0 + DRAW_TW, im.W) - 1, ty1 = min(ty0 + DRAW_TH, im.H) - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = tx0 + lane;
    unsigned col[DRAW_TH / 4];
    unsigned hit = 0;                                                    // bit j: pixel (x, ty0 + wave + 4 j) is painted
    for (int base = im.p0; base < im.p1; base += 256) {
        DrawPrim p;
        bool keep = false;
        if (base + tid < im.p1) {
            p = prims[base + tid];
            // bounding box, branch-free: a glyph's second corner comes from its scale, a segment grows by its reach
            const bool glyph = p.kind == 2;
            const int r = p.kind == 0 ? draw_reach(p.param) : 0;
            const int ex = glyph ? p.x0 + 5 * p.param - 1 : p.x1, ey = glyph ? p.y0 + 7 * p.param - 1 : p.y1;
            const int bx0 = min(p.x0, ex) - r, bx1 = max(p.x0, ex) + r, by0 = min(p.y0, ey) - r, by1 = max(p.y0, ey) + r;
            keep = p.kind >= 0 && p.kind <= 2 && p.param > 0 && bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int pos = __popcll(m & ((1ull << lane) - 1ull)), n = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) pos += s_cnt[w];
            n += s_cnt[w];
        }
        if (keep) s_p[pos] = p;
        __syncthreads();
        if (x < im.W)
            for (int k = 0; k < n; ++k) {
                const DrawPrim q = s_p[k];
#pragma unroll
                for (int j = 0; j < DRAW_TH / 4; ++j)
                    if (draw_covers(q, x, ty0 + wave + 4 * j)) {
                        col[j] = q.color;
                        hit |= 1u << j;
                    }
            }
        __syncthreads();
    }
    if (!hit) return;
#pragma unroll
    for (int j = 0; j < DRAW_TH / 4; ++j) {
        const int y = ty0 + wave + 4 * j;
        if (((hit >> j) & 1u) && y < im.H) {
            unsigned char* o = frames + im.off + ((long)y * im.W + x) * 3;
            o[0] = (unsigned char)(col[j] & 255u);
            o[1] = (unsigned char)((col[j] >> 8) & 255u);
            o[2] = (unsigned char)((col[j] >> 16) & 255u);
        }
    }
}

extern "C" int hn_draw(void* frames, long frames_bytes, const void* imgs, int N, int max_h, int max_w, const void* prims, int nprims,
                       hipStream_t st) {
    HN_CHECK_ARG(frames && imgs && N > 0 && N <= 65535 && max_h > 0 && max_h <= 16384 && max_w > 0 && max_w <= 16384 && frames_bytes > 0 &&
                 nprims >= 0 && (prims || nprims == 0));
    if (nprims == 0) return HN_OK;
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)((max_w + DRAW_TW - 1) / DRAW_TW), (unsigned)((max_h + DRAW_TH - 1) / DRAW_TH), (unsigned)N),
                       dim3(256), 0, st, (unsigned char*)frames, frames_bytes, (const DrawImage*)imgs, (const DrawPrim*)prims, nprims);
    HN_LAUNCH_CHECK();
}
