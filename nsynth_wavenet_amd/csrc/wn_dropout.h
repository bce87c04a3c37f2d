// The dropout mask of the teacher's training forward and reverse passes: a stateless counter hash.
//   keep(seed, site, b, c, t) = word (t & 3) of Philox4x32-10(key = seed, counter = (t >> 2, c, site, b)) >= thr
// with thr = min(2^32 - 1, floor(rate 2^32 + 0.5)) formed once on the host in double.  The bit is a function of these five
// values alone -- not of Tp, tile, chunk, grid or batch size -- so the forward, both reverse passes and the numpy twin
// (nsynth_wavenet_amd/train.py: dropout_keep) agree wherever they evaluate it.  The four words of one counter serve four
// consecutive t of one channel.
#pragma once
#include "wn_codec.h"

// the four words of columns 4 t4 .. 4 t4 + 3 of channel c
__device__ inline void wn_dropout_bits4(uint64_t seed, uint32_t site, uint32_t b, uint32_t c, uint32_t t4, uint32_t (&r)[4]) {
    r[0] = t4; r[1] = c; r[2] = site; r[3] = b;
    wn_philox4x32_10(r, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// bit j of the result: column 4 t4 + j of channel c is kept
__device__ inline unsigned wn_dropout_keep4(uint64_t seed, uint32_t site, uint32_t b, uint32_t c, uint32_t t4, uint32_t thr) {
    uint32_t r[4];
    wn_dropout_bits4(seed, site, b, c, t4, r);
    return (r[0] >= thr ? 1u : 0u) | (r[1] >= thr ? 2u : 0u) | (r[2] >= thr ? 4u : 0u) | (r[3] >= thr ? 8u : 0u);
}
__device__ inline bool wn_dropout_keep(uint64_t seed, uint32_t site, uint32_t b, uint32_t c, long long t, uint32_t thr) {
    return (wn_dropout_keep4(seed, site, b, c, (uint32_t)(t >> 2), thr) >> (unsigned)(t & 3)) & 1u;
}
