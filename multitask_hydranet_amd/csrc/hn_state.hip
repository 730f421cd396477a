// State that a training step writes OUTSIDE the optimizer -- BatchNorm running statistics and their batch counters -- kept in step with
// the decision hn_grad_guard takes about that step, and averaged next to the weights (bn_state.BufferKeeper).
//
// One kernel, three modes, over many small tensors in one launch.  jobs (device): n x {live, shadow, avg, words, first_block, kind}; a
// block = 256 threads x 4 consecutive 32-bit words of one job; block_job: job index of every block (hn_copy_many's idiom).  kind 0: the
// words are fp32 values; kind 1: raw words (an int64 counter is two of them), never read as floats.  A shadow / avg pointer of 0: the job
// has none, and is not touched for it.
//   mode 0  snapshot:  shadow = live                                   (before the forward that will write live)
//   mode 1  settle:    record->skip != 0: live = shadow, else nothing  (after the step's decision)
//   mode 2  settle and average: as mode 1 when skipped (the averages stay untouched, as hn_adam_step_ema leaves e); else
//           kind 0: avg = avg + w * (live - avg) in three rounded operations (ema_lerp_rn), kind 1: avg = live
// Copies move 32-bit words (NaN payloads, -0 and denormals survive), 16 bytes at a time where both pointers of the copy allow.  Every
// thread touches its own words only, reads before it writes, and no workgroup waits on another.
#include "hn_common.h"

__global__ __launch_bounds__(256) void state_guard_kernel(const long* jobs, const int* block_job, int mode, const int* record, float w) {
    const bool skipped = mode != 0 && record != nullptr && record[2] != 0;             // word 2 of hn_grad_guard's record: the skip mask
    if (mode == 1 && !skipped) return;
    const long* jb = jobs + (long)block_job[blockIdx.x] * 6;
    const long n = jb[3];
    const long i0 = (((long)blockIdx.x - jb[4]) * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    unsigned* live = reinterpret_cast<unsigned*>(jb[0]);
    unsigned* shadow = reinterpret_cast<unsigned*>(jb[1]);
    unsigned* avg = reinterpret_cast<unsigned*>(jb[2]);
    if (mode == 2 && !skipped && jb[5] == 0) {
        if (avg == nullptr) return;
        // ONE arithmetic instruction stream for both operand forms (whole aligned float4s / element by element), as in adam_step_kernel
        const float* l = reinterpret_cast<const float*>(live) + i0;
        float* a = reinterpret_cast<float*>(avg) + i0;
        const bool vec = cnt == 4 && ((reinterpret_cast<uintptr_t>(l) | reinterpret_cast<uintptr_t>(a)) & 15) == 0;
        float lv[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(l), y = *reinterpret_cast<const f32x4*>(a);
#pragma unroll
            for (int k = 0; k < 4; ++k) { lv[k] = x[k]; av[k] = y[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) { lv[k] = l[k]; av[k] = a[k]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) av[k] = ema_lerp_rn(av[k], lv[k], w);
        if (vec) {
            *reinterpret_cast<f32x4*>(a) = (f32x4){av[0], av[1], av[2], av[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) a[k] = av[k];
        }
        return;
    }
    // the three word copies: snapshot live -> shadow, restore shadow -> live, a counter's average live -> avg
    const unsigned* src = skipped ? shadow : live;
    unsigned* dst = mode == 0 ? shadow : skipped ? live : avg;
    if (src == nullptr || dst == nullptr) return;                                      // (a job without a shadow / without an average)
    src += i0;
    dst += i0;
    if (cnt == 4 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
    } else {
        for (int k = 0; k < cnt; ++k) dst[k] = src[k];
    }
}

extern "C" int hn_state_guard(const long* jobs, const int* block_job, long total_blocks, int mode, const void* record, double ema_decay,
                              hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0 && total_blocks <= 0x7fffffffL && mode >= 0 && mode <= 2);
    HN_CHECK_ARG(mode != 2 || (ema_decay >= 0.0 && ema_decay < 1.0));                  // (a NaN fails both comparisons)
    if (mode == 1 && record == nullptr) return HN_OK;                                  // "not skipped": a settle without averages writes nothing
    // the average's weight as hn_adam_step_ema forms it: 1 - decay in double, rounded to fp32 once
    const float w = mode == 2 ? (float)(1.0 - ema_decay) : 0.f;
    hipLaunchKernelGGL(state_guard_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, mode,
                       reinterpret_cast<const int*>(record), w);
    HN_LAUNCH_CHECK();
}
