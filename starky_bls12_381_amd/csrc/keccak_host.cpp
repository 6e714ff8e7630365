// Host side of the Keccak hasher (keccak.h; COMPAT.md K1 - K8): keccak256 over bytes, and the challenger's permutation K7 as the
// Fiat-Shamir transcript and the CPU verifier call it.
#include <string.h>

#include "keccak.h"

namespace starkhip {

// K1: rate 136 bytes, padding 0x01 .. 0x80 (original Keccak), 32 bytes out
void keccak256_host(const uint8_t* bytes, size_t len, uint8_t out[32]) {
    uint64_t a[25] = {0};
    const size_t rate = 8 * KECCAK_RATE_WORDS;
    uint8_t block[8 * KECCAK_RATE_WORDS];
    for (bool last = false; !last;) {
        const size_t take = len < rate ? len : rate;
        last = take < rate;
        memset(block, 0, sizeof block);
        if (take) memcpy(block, bytes, take);
        if (last) {
            block[take] ^= 0x01;
            block[rate - 1] ^= 0x80;
        }
        for (int i = 0; i < KECCAK_RATE_WORDS; i++) {
            uint64_t w = 0;
            for (int b = 0; b < 8; b++) w |= (uint64_t)block[8 * i + b] << (8 * b);
            a[i] ^= w;
        }
        keccak_f1600(a);
        bytes += take;
        len -= take;
    }
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(a[i] >> (8 * b));
}

void keccak_permute_host(gl_t* s) { keccak_permute(s); }

}  // namespace starkhip
