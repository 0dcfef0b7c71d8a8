// The counter-based generator of the disturbed plants' kicks (srb_plant.hip, srb12_plant.hip): one copy for both modes,
// so a LIP rollout and an SRB-12 rollout with one seed draw the same words.
#pragma once

// Philox4x32-10 (Salmon et al., SC'11; Random123): counter (c0, c1, c2, c3), key (k0, k1) -> four words
__device__ __forceinline__ void plant_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                             unsigned w[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * (unsigned long long)c0, p1 = 0xCD9E8D57ull * (unsigned long long)c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// a word as a uniform draw in (-1, 1), never 0: ((double)(int32_t)w + 0.5) * 2^-31, every step exact
__device__ __forceinline__ double plant_uniform(unsigned w) { return ((double)(int)w + 0.5) * 0x1p-31; }
