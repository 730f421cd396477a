// Full-state training checkpoints (checkpoint.StatePacker): every tensor of the training state gathered into ONE staging
// buffer, checksummed, verified and scattered back in place -- one launch over ~3 300 tensors instead of one synchronising copy each.
//
// jobs (device): n x {src, dst, words, first_block}; a block = 256 threads x 4 consecutive 32-bit WORDS of one job; block_job: job index
// of every block (hn_copy_many's idiom).  Words are moved, never floats: NaN payloads, -0, denormals and int64 counters (two words)
// arrive as they are.  Whole 16-byte vectors where the pointers of the job allow, single words otherwise, into the same four registers:
// what is summed and what is stored does not depend on alignment.
//
// Checksum of a job with words w[0 .. W-1], each a uint32 zero-extended to 64 bits:  s1 = sum w[i],  s2 = sum (i + 1) * w[i],  both
// mod 2^64.  Integer arithmetic: the result cannot depend on the order of the additions.  It is formed as hn_grad_guard forms its
// sums, without atomics: ckpt_block_kernel leaves one {s1, s2} partial per block in the caller's workspace (every block writes its
// own: nothing has to be zeroed), ckpt_job_kernel folds a job's partials with one workgroup, and for a verification ckpt_verdict_kernel
// compares all jobs with one workgroup and writes the whole verdict.  No workgroup waits on another.
//
//   COPY  SUM  GUARDED
//    1     1     0      hn_state_pack:    dst = src, sums of the words read
//    0     1     0      hn_state_verify:  sums of src only
//    1     0     1      hn_state_unpack:  every thread reads verdict[0] first; non-zero: return before the first store
#include "hn_common.h"

typedef unsigned long long u64;

template <bool COPY, bool SUM, bool GUARDED>
__global__ __launch_bounds__(256) void ckpt_block_kernel(const long* jobs, const int* block_job, u64* partial, const int* verdict) {
    if constexpr (GUARDED) {
        if (verdict != nullptr && verdict[0] != 0) return;
    }
    const long* jb = jobs + (long)block_job[blockIdx.x] * 4;
    const long n = jb[2];
    const long i0 = (((long)blockIdx.x - jb[3]) * 256 + threadIdx.x) * 4;
    const int cnt = i0 >= n ? 0 : (n - i0 < 4 ? (int)(n - i0) : 4);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (cnt > 0) {
        const unsigned* src = reinterpret_cast<const unsigned*>(jb[0]) + i0;
        if (cnt == 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(src);
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = x[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) w[k] = src[k];
        }
        if constexpr (COPY) {
            unsigned* dst = reinterpret_cast<unsigned*>(jb[1]) + i0;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                *reinterpret_cast<u32x4*>(dst) = (u32x4){w[0], w[1], w[2], w[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) dst[k] = w[k];
            }
        }
    }
    if constexpr (SUM) {
        // absent words are 0 and add nothing; (i + 1) is the word's 1-based index within its JOB
        __shared__ u64 red[8];
        u64 s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s1 += (u64)w[k];
            s2 += (u64)(i0 + k + 1) * (u64)w[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o);
            s2 += __shfl_xor(s2, o);
        }
        if ((threadIdx.x & 63) == 0) {
            red[(threadIdx.x >> 6) * 2] = s1;
            red[(threadIdx.x >> 6) * 2 + 1] = s2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            partial[(long)blockIdx.x * 2] = red[0] + red[2] + red[4] + red[6];
            partial[(long)blockIdx.x * 2 + 1] = red[1] + red[3] + red[5] + red[7];
        }
    }
}

// one workgroup per job: thread t adds the partials of the job's blocks t, t + 256, ...; then the workgroup's sum
__global__ __launch_bounds__(256) void ckpt_job_kernel(const long* jobs, const u64* partial, u64* sums) {
    __shared__ u64 red[8];
    const long* jb = jobs + (long)blockIdx.x * 4;
    const long nb = (jb[2] + 1023) / 1024;
    const u64* pp = partial + jb[3] * 2;
    u64 s1 = 0, s2 = 0;
    for (long b = threadIdx.x; b < nb; b += 256) {
        s1 += pp[b * 2];
        s2 += pp[b * 2 + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[(threadIdx.x >> 6) * 2] = s1;
        red[(threadIdx.x >> 6) * 2 + 1] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[(long)blockIdx.x * 2] = red[0] + red[2] + red[4] + red[6];
        sums[(long)blockIdx.x * 2 + 1] = red[1] + red[3] + red[5] + red[7];
    }
}

// one workgroup: how many jobs' sums differ from what is expected, and the first of them; all four words of the verdict are written
__global__ __launch_bounds__(256) void ckpt_verdict_kernel(const u64* sums, const u64* expect, long n_jobs, int* verdict) {
    __shared__ int red[8];
    int bad = 0, first = 0x7fffffff;
    for (long j = threadIdx.x; j < n_jobs; j += 256)
        if (sums[j * 2] != expect[j * 2] || sums[j * 2 + 1] != expect[j * 2 + 1]) {
            bad += 1;
            if ((int)j < first) first = (int)j;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o);
        const int f = __shfl_xor(first, o);
        first = f < first ? f : first;
    }
    if ((threadIdx.x & 63) == 0) {
        red[(threadIdx.x >> 6) * 2] = bad;
        red[(threadIdx.x >> 6) * 2 + 1] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0, f = 0x7fffffff;
        for (int k = 0; k < 4; ++k) {
            b += red[k * 2];
            f = red[k * 2 + 1] < f ? red[k * 2 + 1] : f;
        }
        verdict[0] = b;
        verdict[1] = b ? f : -1;
        verdict[2] = 0;
        verdict[3] = 0;
    }
}

static inline bool ckpt_tables_ok(const long* jobs, const int* block_job, long total_blocks) {
    return jobs && block_job && total_blocks > 0 && total_blocks <= 0x7fffffffL;
}

extern "C" int hn_state_pack(const long* jobs, const int* block_job, long total_blocks, long n_jobs, void* ws, void* sums, hipStream_t st) {
    HN_CHECK_ARG(ckpt_tables_ok(jobs, block_job, total_blocks) && n_jobs > 0 && n_jobs <= 0x7fffffffL && ws && sums &&
                 ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(sums)) & 7) == 0);
    hipLaunchKernelGGL((ckpt_block_kernel<true, true, false>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, (u64*)ws,
                       (const int*)nullptr);
    hipLaunchKernelGGL(ckpt_job_kernel, dim3((unsigned)n_jobs), dim3(256), 0, st, jobs, (const u64*)ws, (u64*)sums);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_state_verify(const long* jobs, const int* block_job, long total_blocks, long n_jobs, const void* expect, void* ws,
                               void* sums, int* verdict, hipStream_t st) {
    HN_CHECK_ARG(ckpt_tables_ok(jobs, block_job, total_blocks) && n_jobs > 0 && n_jobs <= 0x7fffffffL && expect && ws && sums && verdict &&
                 ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(expect)) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(verdict) & 3) == 0);
    hipLaunchKernelGGL((ckpt_block_kernel<false, true, false>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, (u64*)ws,
                       (const int*)nullptr);
    hipLaunchKernelGGL(ckpt_job_kernel, dim3((unsigned)n_jobs), dim3(256), 0, st, jobs, (const u64*)ws, (u64*)sums);
    hipLaunchKernelGGL(ckpt_verdict_kernel, dim3(1), dim3(256), 0, st, (const u64*)sums, (const u64*)expect, n_jobs, verdict);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_state_unpack(const long* jobs, const int* block_job, long total_blocks, const int* verdict, hipStream_t st) {
    HN_CHECK_ARG(ckpt_tables_ok(jobs, block_job, total_blocks) && (reinterpret_cast<uintptr_t>(verdict) & 3) == 0);
    hipLaunchKernelGGL((ckpt_block_kernel<true, false, true>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, (u64*)nullptr,
                       verdict);
    HN_LAUNCH_CHECK();
}

// the same two sums on the host, no GPU call: checks a file where there is no device, and pins the definition on the CPU
extern "C" int hn_state_checksum_host(const void* words, long n_words, unsigned long long* out) {
    HN_CHECK_ARG(out && n_words >= 0 && (words || n_words == 0) && (reinterpret_cast<uintptr_t>(words) & 3) == 0);
    const uint32_t* w = static_cast<const uint32_t*>(words);
    u64 s1 = 0, s2 = 0;
    for (long i = 0; i < n_words; ++i) {
        s1 += (u64)w[i];
        s2 += (u64)(i + 1) * (u64)w[i];
    }
    out[0] = s1;
    out[1] = s2;
    return HN_OK;
}
