// gram_item.hpp -- the item of the batched Gram kernels, shared by the launch declarations (kernels.hpp) and the device-side tile machinery (mfma_common.hpp)
#pragma once

namespace tnqs {

struct GramItem {         // partial[c][i + KK*j] = sum_{(a,b) in chunk c} X[i,(a,b)] * conj(Y[j,(a,b)]),  i,j = (s,k)
    const void* X; const void* Y; void* partial;
    int D, PA, K, PB;
    int TA, TB, nta, ntb;
    int chunk_begin, nchunks, tiles_per_chunk;
    const void* M;        // fused variant only: 32 x 32 message absorbed on the first row leg of X before the Gram
};

}  // namespace tnqs
