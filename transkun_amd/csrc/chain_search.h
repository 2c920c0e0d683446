// chain_search.h -- which chain owns a row of the packed interval layout (pairs [K][2] + offsets [C+1], chain order)
#pragma once
#include "common.h"

namespace semicrf {

__device__ __forceinline__ int chain_of_interval(const int* __restrict__ offsets, int C, int i)
{
    int lo = 0, hi = C;                       // largest c with offsets[c] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace semicrf
