// Batched AEAD for gfx950: ChaCha20-Poly1305 (RFC 8439) and AES-256-GCM (NIST SP 800-38D, 96-bit
// IV, 128-bit tag), one lane per message.
//
// Replaces, for N sessions at once, the two calls the reference makes with every derived session
// key: SymmetricAlgorithm.encrypt / decrypt (quantum_resistant_p2p/crypto/symmetric.py:95-161,
// 193-259), first for the key_exchange_test message that completes a handshake
// (app/messaging.py:1102-1114 sealed, :1224-1250 opened) and then for every message (:1465, :1645).
// A sealed row is nonce (12) || ciphertext || tag (16), the bytes `encrypt` returns (:116-119).
//
// These messages are tens to hundreds of bytes, each with its own key, offset and length, so like
// k_hkdf_sha256 the kernels are latency-bound, not VALU- or bandwidth-bound: bytes are gathered with
// byte loads from per-message offsets and every lane walks its own message serially.  Long rows have
// their own kernels, aead_long.hip; the device functions both use are in aead_dev.cuh.
//
// State lives in registers: the 16 ChaCha words (every rotation one v_alignbit_b32), Poly1305 in
// five 26-bit limbs with 64-bit products, the 60 AES-256 round-key words, H and the GHASH
// accumulator.  No kernel writes key material (round keys, H, the Poly1305 one-time key) to global
// memory, so there is no scratch to wipe; keys are read from the caller's buffer and never passed
// as kernel arguments (key hygiene).
//
// AES uses the LDS-replicated T-table of aes.cuh (Lds2).  Here the key is secret (FrodoKEM's seedA
// is public), and the replicated layout is what makes that acceptable: entry x of lane l lives at
// dword 64 x + (l & 31) (+ 32 for T2), so whatever the index every lane of a 32-lane group reads its
// own bank -- one LDS cycle per group for every access, no bank conflict whose cost could depend on
// key or state bytes.  The key schedule's SubWord goes through the same table (the S-box is byte 1
// of T0), not through the constant-memory S-box.  GHASH multiplies bit-serially with masks: no
// branch and no table index depends on H or on the data.  Tags are compared without early exit
// (OR-accumulated, as k_keys_equal) and Open writes plaintext only where the tag matches.
#include "aead_dev.cuh"

namespace qrk {
namespace aead {

// sealed row i = nonce | ct | tag at byte pt_off[i] + 28 i.  `sealed` is read back (this lane's own
// ciphertext bytes, for the tag), so it is not __restrict__.
__global__ __launch_bounds__(256) void k_chacha_seal(size_t n, const uint8_t* __restrict__ keys,
                                                     const uint8_t* __restrict__ nonces,
                                                     const uint8_t* __restrict__ pt,
                                                     const uint64_t* __restrict__ pt_off,
                                                     const uint8_t* __restrict__ aad,
                                                     const uint64_t* __restrict__ aad_off, uint32_t aad_len,
                                                     uint8_t* sealed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = pt_off[i], l64 = pt_off[i + 1] - o;
  const Span ad = span_of(aad, aad_off, aad_len, i);
  if (l64 >= ROW_MAX || !ad.ok) return;
  const uint32_t len = (uint32_t)l64;
  uint8_t* row = sealed + o + OVERHEAD * i;
  const ChaKey K = chacha_key(keys + 32 * i, nonces + NONCE * i);
#pragma unroll
  for (int t = 0; t < 3; ++t) scatter32(row, 4 * t, NONCE, K.n[t]);
  chacha_xor(K, pt + o, row + NONCE, len, ~0u);
  uint32_t tag[4];
  chacha_tag(K, ad, row + NONCE, len, tag);
#pragma unroll
  for (int t = 0; t < 4; ++t) scatter32(row + NONCE + len, 4 * t, TAG, tag[t]);
}

// plaintext i at byte sealed_off[i] - 28 i; status[i] = 0, or -1 (short row, oversize row, bad tag)
__global__ __launch_bounds__(256) void k_chacha_open(size_t n, const uint8_t* __restrict__ keys,
                                                     const uint8_t* __restrict__ sealed,
                                                     const uint64_t* __restrict__ sealed_off,
                                                     const uint8_t* __restrict__ aad,
                                                     const uint64_t* __restrict__ aad_off, uint32_t aad_len,
                                                     uint8_t* __restrict__ pt, int32_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = sealed_off[i], l64 = sealed_off[i + 1] - o;
  const Span ad = span_of(aad, aad_off, aad_len, i);
  // (o < 28 i: rows before this one were shorter than 28 bytes and its plaintext has no place)
  if (l64 < OVERHEAD || l64 >= ROW_MAX || !ad.ok || o < (uint64_t)OVERHEAD * i) {
    status[i] = -1;
    return;
  }
  const uint32_t len = (uint32_t)l64 - OVERHEAD;
  const uint8_t* row = sealed + o;
  const ChaKey K = chacha_key(keys + 32 * i, row);
  uint32_t tag[4], d = 0;
  chacha_tag(K, ad, row + NONCE, len, tag);
#pragma unroll
  for (int t = 0; t < 4; ++t) d |= tag[t] ^ load32(row + NONCE + len + 4 * t);
  const bool ok = d == 0;
  chacha_xor(K, row + NONCE, pt + (o - OVERHEAD * i), len, ok ? ~0u : 0u);
  status[i] = ok ? 0 : -1;
}

// tests: tag_i = Poly1305(key32_i = r | s, msg_i), any message length (RFC 8439 section 2.5.1: a
// short last block gets its 0x01 byte and no 2^128 bit)
__global__ __launch_bounds__(256) void k_dbg_poly1305(size_t n, const uint8_t* __restrict__ key32,
                                                      const uint8_t* __restrict__ msg,
                                                      const uint64_t* __restrict__ msg_off,
                                                      uint8_t* __restrict__ tag) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = msg_off[i], l64 = msg_off[i + 1] - o;
  if (l64 >= ROW_MAX) return;
  const uint32_t len = (uint32_t)l64, full = len & ~15u, rem = len & 15u;
  uint32_t k[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) k[t] = load32(key32 + 32 * i + 4 * t);
  Poly P;
  P.init(k);
  P.absorb_padded(msg + o, full);
  if (rem) {
    uint32_t m[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      m[t] = gather32(msg + o, full + 4 * t, len);
      if ((rem >> 2) == (uint32_t)t) m[t] |= 1u << (8 * (rem & 3));
    }
    P.block(m, 0);
  }
  uint32_t out[4];
  P.finish(out);
#pragma unroll
  for (int t = 0; t < 4; ++t) scatter32(tag + 16 * i, 4 * t, TAG, out[t]);
}

__global__ __launch_bounds__(256) void k_gcm_seal(size_t n, const uint8_t* __restrict__ keys,
                                                  const uint8_t* __restrict__ nonces,
                                                  const uint8_t* __restrict__ pt,
                                                  const uint64_t* __restrict__ pt_off,
                                                  const uint8_t* __restrict__ aad,
                                                  const uint64_t* __restrict__ aad_off, uint32_t aad_len,
                                                  uint8_t* sealed) {
  QRK_AEAD_LDS_TABLE();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = pt_off[i], l64 = pt_off[i + 1] - o;
  const Span ad = span_of(aad, aad_off, aad_len, i);
  if (l64 >= ROW_MAX || !ad.ok) return;
  const uint32_t len = (uint32_t)l64;
  uint8_t* row = sealed + o + OVERHEAD * i;
  Gcm G;
  G.init(L, keys + 32 * i, nonces + NONCE * i);
#pragma unroll
  for (int t = 0; t < 3; ++t) scatter32(row, 4 * t, NONCE, G.iv[t]);
  G.ctr_xor(L, pt + o, row + NONCE, len, ~0u);
  uint32_t tag[4];
  G.tag(L, ad, row + NONCE, len, tag);
#pragma unroll
  for (int t = 0; t < 4; ++t) scatter32(row + NONCE + len, 4 * t, TAG, tag[t]);
}

__global__ __launch_bounds__(256) void k_gcm_open(size_t n, const uint8_t* __restrict__ keys,
                                                  const uint8_t* __restrict__ sealed,
                                                  const uint64_t* __restrict__ sealed_off,
                                                  const uint8_t* __restrict__ aad,
                                                  const uint64_t* __restrict__ aad_off, uint32_t aad_len,
                                                  uint8_t* __restrict__ pt, int32_t* __restrict__ status) {
  QRK_AEAD_LDS_TABLE();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = sealed_off[i], l64 = sealed_off[i + 1] - o;
  const Span ad = span_of(aad, aad_off, aad_len, i);
  // (o < 28 i: rows before this one were shorter than 28 bytes and its plaintext has no place)
  if (l64 < OVERHEAD || l64 >= ROW_MAX || !ad.ok || o < (uint64_t)OVERHEAD * i) {
    status[i] = -1;
    return;
  }
  const uint32_t len = (uint32_t)l64 - OVERHEAD;
  const uint8_t* row = sealed + o;
  Gcm G;
  G.init(L, keys + 32 * i, row);
  uint32_t tag[4], d = 0;
  G.tag(L, ad, row + NONCE, len, tag);
#pragma unroll
  for (int t = 0; t < 4; ++t) d |= tag[t] ^ load32(row + NONCE + len + 4 * t);
  const bool ok = d == 0;
  G.ctr_xor(L, row + NONCE, pt + (o - OVERHEAD * i), len, ok ? ~0u : 0u);
  status[i] = ok ? 0 : -1;
}

// tests: out_i = GHASH_{h_i}(data_i), data_i a whole number of blocks
__global__ __launch_bounds__(256) void k_dbg_ghash(size_t n, const uint8_t* __restrict__ h,
                                                   const uint8_t* __restrict__ data,
                                                   const uint64_t* __restrict__ data_off, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = data_off[i], l64 = data_off[i + 1] - o;
  if (l64 >= ROW_MAX) return;
  uint32_t hw[4], y[4] = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) hw[t] = bswap(load32(h + 16 * i + 4 * t));
  ghash_padded(y, hw, data + o, (uint32_t)l64 & ~15u);
#pragma unroll
  for (int t = 0; t < 4; ++t) scatter32(out + 16 * i, 4 * t, TAG, bswap(y[t]));
}

}  // namespace aead

static dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

hipError_t aead_seal(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* nonces, const uint8_t* pt,
                     const uint64_t* pt_off, const uint8_t* aad, const uint64_t* aad_off, size_t aad_len,
                     uint8_t* sealed, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (aad_len >= aead::ROW_MAX) return hipErrorInvalidValue;
  if (alg == AeadAlg::CHACHA20_POLY1305)
    QRK_LAUNCH("k_chacha_seal", st, aead::k_chacha_seal, grid_of(n), dim3(256), 0, st, n, keys, nonces, pt, pt_off, aad,
               aad_off, (uint32_t)aad_len, sealed);
  else
    QRK_LAUNCH("k_gcm_seal", st, aead::k_gcm_seal, grid_of(n), dim3(256), 0, st, n, keys, nonces, pt, pt_off, aad,
               aad_off, (uint32_t)aad_len, sealed);
  return launch_status();
}

hipError_t aead_open(AeadAlg alg, size_t n, const uint8_t* keys, const uint8_t* sealed, const uint64_t* sealed_off,
                     const uint8_t* aad, const uint64_t* aad_off, size_t aad_len, uint8_t* pt, int32_t* status,
                     hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (aad_len >= aead::ROW_MAX) return hipErrorInvalidValue;
  if (alg == AeadAlg::CHACHA20_POLY1305)
    QRK_LAUNCH("k_chacha_open", st, aead::k_chacha_open, grid_of(n), dim3(256), 0, st, n, keys, sealed, sealed_off, aad,
               aad_off, (uint32_t)aad_len, pt, status);
  else
    QRK_LAUNCH("k_gcm_open", st, aead::k_gcm_open, grid_of(n), dim3(256), 0, st, n, keys, sealed, sealed_off, aad,
               aad_off, (uint32_t)aad_len, pt, status);
  return launch_status();
}

hipError_t dbg_poly1305(size_t n, const uint8_t* key32, const uint8_t* msg, const uint64_t* msg_off, uint8_t* tag,
                        hipStream_t st) {
  if (n == 0) return hipSuccess;
  QRK_LAUNCH("k_dbg_poly1305", st, aead::k_dbg_poly1305, grid_of(n), dim3(256), 0, st, n, key32, msg, msg_off, tag);
  return launch_status();
}

hipError_t dbg_ghash(size_t n, const uint8_t* h, const uint8_t* data, const uint64_t* data_off, uint8_t* out,
                     hipStream_t st) {
  if (n == 0) return hipSuccess;
  QRK_LAUNCH("k_dbg_ghash", st, aead::k_dbg_ghash, grid_of(n), dim3(256), 0, st, n, h, data, data_off, out);
  return launch_status();
}

}  // namespace qrk
