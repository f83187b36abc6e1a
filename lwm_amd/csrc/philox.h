// philox.h -- the counter-based generator shared by the token sampler (sample.h) and the dropout kernels (dropout.h).
// Expects wave_ops.h (the product's or the host emulation's) to be included first.
#pragma once

namespace lwm {

// Philox4x32-10 (Salmon et al., SC'11): the round constants and key schedule of rocRAND's philox4x32_10_engine.
LWM_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
    }
}

}  // namespace lwm
