// Gradient accumulation over several backward passes (train.accum_steps; optim.GradAccumulator): the running MEAN of the
// micro-batches' gradients, of up to 8 loss scalars, and a sticky word that remembers a bad loss or a raised status word of any
// micro-batch of the group -- one launch per micro-batch over all gradient tensors.
//
// jobs (device): n x {g, acc, numel, first_block}; a block = 256 threads x 4 consecutive elements of one tensor; block_job: job index of
// every block (hn_copy_many's idiom).  j = 1-based index of the micro-batch in its group, w = (float)(1.0 / j):
//   j == 1:  acc = g                          (acc is NOT read: what an earlier group, or nobody, left there cannot leak)
//   j  > 1:  acc = acc + w * (g - acc)        in three rounded operations (ema_lerp_rn, as hn_adam_step_ema and hn_state_guard)
// so after every launch acc is the mean of the micro-batches seen so far.  Whole float4s where g and acc are both 16-byte aligned, single
// elements otherwise, through ONE arithmetic instruction stream.  Every thread touches its own elements only and reads before it writes;
// no workgroup waits on another.  Thread 0 of block 0 also keeps the loss means (same rule) and the sticky word, with plain stores.
#include "hn_common.h"

struct AccumTail {
    int n_losses, n_words;
    const float* losses[8];
    const int* words[4];
    float* loss_mean;
    int* sticky;
};

template <bool FIRST>
__global__ __launch_bounds__(256) void grad_accum_kernel(const long* jobs, const int* block_job, float w, AccumTail t) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int bits = 0;
        for (int i = 0; i < t.n_losses; ++i) {
            const float l = t.losses[i][0];
            if (!(fabsf(l) <= __FLT_MAX__)) bits |= 2;
            t.loss_mean[i] = FIRST ? l : ema_lerp_rn(t.loss_mean[i], l, w);
        }
        for (int i = 0; i < t.n_words; ++i)
            if (t.words[i][0] != 0) bits |= 4;
        if (t.sticky) t.sticky[0] = FIRST ? bits : (t.sticky[0] | bits);
    }
    const long* jb = jobs + (long)block_job[blockIdx.x] * 4;
    const long n = jb[2];
    const long i0 = (((long)blockIdx.x - jb[3]) * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    const float* g = reinterpret_cast<const float*>(jb[0]) + i0;
    float* a = reinterpret_cast<float*>(jb[1]) + i0;
    const bool vec = cnt == 4 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(a)) & 15) == 0;
    if constexpr (FIRST) {
        // a copy of 32-bit words, not of floats: NaN payloads, -0 and denormals of g arrive as they are
        const unsigned* s = reinterpret_cast<const unsigned*>(g);
        unsigned* d = reinterpret_cast<unsigned*>(a);
        if (vec) {
            *reinterpret_cast<u32x4*>(d) = *reinterpret_cast<const u32x4*>(s);
        } else {
            for (int k = 0; k < cnt; ++k) d[k] = s[k];
        }
        return;
    }
    float gv[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(g), y = *reinterpret_cast<const f32x4*>(a);
#pragma unroll
        for (int k = 0; k < 4; ++k) { gv[k] = x[k]; av[k] = y[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) { gv[k] = g[k]; av[k] = a[k]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) av[k] = ema_lerp_rn(av[k], gv[k], w);
    if (vec) {
        *reinterpret_cast<f32x4*>(a) = (f32x4){av[0], av[1], av[2], av[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) a[k] = av[k];
    }
}

extern "C" int hn_grad_accum(const long* jobs, const int* block_job, long total_blocks, long j, const void* const* losses, int n_losses,
                             float* loss_mean, const void* const* words, int n_words, int* sticky, hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0 && total_blocks <= 0x7fffffffL && j >= 1 && n_losses >= 0 && n_losses <= 8 &&
                 n_words >= 0 && n_words <= 4 && (n_losses == 0 || (losses && loss_mean)) && (n_words == 0 || words) &&
                 ((n_losses == 0 && n_words == 0) || sticky));
    AccumTail t = {};
    for (int i = 0; i < n_losses; ++i) { HN_CHECK_ARG(losses[i]); t.losses[i] = (const float*)losses[i]; }
    for (int i = 0; i < n_words; ++i) { HN_CHECK_ARG(words[i]); t.words[i] = (const int*)words[i]; }
    t.n_losses = n_losses; t.n_words = n_words; t.loss_mean = loss_mean; t.sticky = sticky;
    // the mean's weight: 1 / j in double, rounded to fp32 once
    const float w = (float)(1.0 / (double)j);
    if (j == 1) hipLaunchKernelGGL(grad_accum_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, w, t);
    else hipLaunchKernelGGL(grad_accum_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, w, t);
    HN_LAUNCH_CHECK();
}
