// Host side of the KeyGenerator / Encryptor randomness (defined in hec_seal_io.cpp beside SEAL's PRNG stream; plain
// C++, no device code): the seed derivation and the redraw walk of the uniform sampler.
#pragma once
#include <cstdint>

namespace hec_host {
// 64 bytes from getrandom(2); false when the system call fails (there is no fallback)
bool entropy_seed(uint64_t out[8]);
// sub(call, role, i, j) = BLAKE2Xb(input = the four values as little-endian u64, key = seed, 64 bytes)
void sub_seed(const uint64_t seed[8], uint64_t call, uint64_t role, uint64_t i, uint64_t j, uint64_t out[8]);
// The redraws of one stream whose first nwords words went through sample_poly_uniform's bulk draw: pos[0 .. n) are the
// rejected word positions in ascending order, the modulus of position p is q[p / N]; each is redrawn from the
// stream's continuation until accepted, exactly as the host routine walks them; val[k] = the accepted word mod q.
void redraw_walk(const uint64_t sub[8], uint64_t nwords, uint64_t N, const uint64_t *q, const uint64_t *pos,
                 uint64_t n, uint64_t *val);
}  // namespace hec_host
