// One wave's sweep over the C columns of a row, shared by the cross-entropy kernel (loss.hip) and the token-score
// kernel (score.hip).  Lane l owns the columns l mod 64.  The body has four trips' loads in flight (c, c + 64,
// c + 128, c + 192 while c + 192 < C; left alone, hipcc waits for every load before it issues the next), then calls
// f(value, column) in ascending column order; the tail steps by 64.  So whatever f accumulates, it accumulates per
// lane in ascending trips -- the order the fp32 emulations of the tests (row_kernel_cases.row_sum) assume.  4-byte
// loads only: column c stays on lane c % 64 whatever the row's alignment (C = 513 rows are 4-byte aligned).
#pragma once

namespace qarig {

template <class F>
__device__ __forceinline__ void row_sweep(const float* __restrict__ x, int C, int lane, F&& f) {
    int c = lane;
    for (; c + 192 < C; c += 256) {
        const float v0 = x[c], v1 = x[c + 64], v2 = x[c + 128], v3 = x[c + 192];
        f(v0, c);
        f(v1, c + 64);
        f(v2, c + 128);
        f(v3, c + 192);
    }
    for (; c < C; c += 64) f(x[c], c);
}

}  // namespace qarig
