// fold_reduce_check -- the folded column reduction on the device, on the caller's columns (tests/test_gpu_fold_reduce_block.py).
// A program of its own that compiles the product's definitions: colacc_fold<false> and colacc_fold<true> of csrc/stage_a_common.h
// and colacc_fold_to_4q of csrc/ntt16_kernel.h (the same block on the transform's fixed registers).  It judges nothing: the test
// compares every word with tests/fold_reduce.py.
//
//   fold_reduce_check IN OUT n d_0 d_1 ...
// IN:  [nd][n][3] 64-bit words, the columns (c0, c1, c2) of the n cases of every d;  OUT: [nd][n][3] words: lazy, canonical, ntt16's lazy.
// One launch per d: the modulus is wave-uniform (scalar operands), as in the kernels.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "stage_a_common.h"
#include "ntt16_kernel.h"

using piehip::u32;
using piehip::u64;

__global__ void __launch_bounds__(64) fold_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u32 n, u64 nq)
{
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const piehip::ColAcc a = {in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]};
    out[3 * (size_t)i] = piehip::colacc_fold<false>(a, nq);
    out[3 * (size_t)i + 1] = piehip::colacc_fold<true>(a, nq);
    out[3 * (size_t)i + 2] = piehip::ntt16::colacc_fold_to_4q(a.c0, a.c1, a.c2, nq);
}

#define FR_HIP(expr)                                                                                \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "fold_reduce_check: %s: %s\n", #expr, hipGetErrorString(e_));           \
            return 3;                                                                               \
        }                                                                                           \
    } while (0)

int main(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: fold_reduce_check IN OUT n d_0 [d_1 ...]\n");
        return 2;
    }
    const u32 n = (u32)strtoul(argv[3], nullptr, 10);
    const size_t nd = (size_t)argc - 4;
    if (!n || n > (1u << 20)) {
        fprintf(stderr, "fold_reduce_check: n out of range\n");
        return 2;
    }
    std::vector<u64> in(nd * n * 3), out(nd * n * 3);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(in.data(), sizeof(u64), in.size(), f) != in.size()) {
        fprintf(stderr, "fold_reduce_check: %s: fewer than %zu words\n", argv[1], in.size());
        return 2;
    }
    fclose(f);
    u64 *d_in = nullptr, *d_out = nullptr;
    FR_HIP(hipMalloc(&d_in, (size_t)n * 3 * sizeof(u64)));
    FR_HIP(hipMalloc(&d_out, (size_t)n * 3 * sizeof(u64)));
    for (size_t k = 0; k < nd; k++) {
        const u64 d = strtoull(argv[4 + k], nullptr, 10);
        if (!d || d >= (1ull << 28)) {
            fprintf(stderr, "fold_reduce_check: d out of range\n");
            return 2;
        }
        const u64 nq = 0 - ((1ull << 60) - d);   // 2^64 - q: the low word is d
        FR_HIP(hipMemcpy(d_in, in.data() + k * n * 3, (size_t)n * 3 * sizeof(u64), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(fold_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n, nq);
        FR_HIP(hipGetLastError());
        FR_HIP(hipMemcpy(out.data() + k * n * 3, d_out, (size_t)n * 3 * sizeof(u64), hipMemcpyDeviceToHost));
    }
    FR_HIP(hipFree(d_in));
    FR_HIP(hipFree(d_out));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(u64), out.size(), f) != out.size() || fclose(f)) {
        fprintf(stderr, "fold_reduce_check: cannot write %s\n", argv[2]);
        return 2;
    }
    printf("fold_reduce_check: %zu moduli, %u cases each\n", nd, n);
    return 0;
}
