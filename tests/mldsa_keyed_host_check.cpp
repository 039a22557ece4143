// Stand-alone host-memory check of the ML-DSA key-set entry points of csrc/abi_sig.cpp: every path that returns
// before any GPU work (load, info, argument refusals, free), meant to be built with the host sanitizers and run on
// a machine without a GPU.  From the repository root:
//
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude"
//   hipcc $F -c tests/mldsa_keyed_host_check.cpp -o build/host_check.o
//   for f in ctx kem aead sig util; do
//     hipcc $F -fPIC -c quantum-resistant-p2p_amd/csrc/abi_$f.cpp -o build/abi_${f}_san.o; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/host_check.o build/abi_*_san.o \
//         build/qrkem/{mlkem,util,frodo,hkdf,wire,hqc,aead,mldsa,mldsa_sign,mldsa_keyed,slhdsa,slhdsa_sign}.o \
//         -o build/mldsa_keyed_host_check && build/mldsa_keyed_host_check
//
// (the kernel objects come from `make -C quantum-resistant-p2p_amd/csrc`; only the abi_*.cpp files and this file are
// instrumented).  Prints "ok" and exits 0; any sanitizer report or failed expectation exits nonzero.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qrkem.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
  do {                                                                            \
    if (!(cond)) {                                                                \
      std::fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, qrk_last_error()); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

static bool says(const char* what) { return std::strstr(qrk_last_error(), what) != nullptr; }

int main() {
  qrk_ctx* fake = (qrk_ctx*)(uintptr_t)1;  // never dereferenced: every call below is refused before the context is used
  uint8_t* keys = (uint8_t*)std::malloc(4896);
  std::memset(keys, 0, 4896);
  const char* names[3] = {"ML-DSA-44", "ML-DSA-65", "ML-DSA-87"};
  int (*loaders[2])(qrk_ctx*, const char*, size_t, const uint8_t*, qrk_mldsa_keyset**, void*) = {
      qrk_mldsa_pubkeys_load, qrk_mldsa_seckeys_load};
  for (auto load : loaders) {
    for (const char* name : names) {
      qrk_mldsa_keyset* ks = nullptr;
      EXPECT(load(nullptr, name, 1, keys, &ks, nullptr) == -1 && says("null context"));
      EXPECT(load(fake, name, 0, keys, &ks, nullptr) == -1 && says("at least one key"));
      EXPECT(load(fake, name, 1, nullptr, &ks, nullptr) == -1 && says("null buffer"));
      EXPECT(load(fake, name, 1, keys, nullptr, nullptr) == -1 && says("null buffer"));
      EXPECT(load(fake, name, (size_t)1 << 40, keys, &ks, nullptr) == -1 && says("scratch budget"));
      EXPECT(load(fake, name, ~(size_t)0, keys, &ks, nullptr) == -1 && says("scratch budget"));
      EXPECT(ks == nullptr);
    }
    const char* others[5] = {"ML-KEM-768", "SLH-DSA-SHA2-128f", "SPHINCS+-SHA2-256f-simple", "", nullptr};
    for (const char* name : others) {
      qrk_mldsa_keyset* ks = nullptr;
      EXPECT(load(fake, name, 1, keys, &ks, nullptr) == -1 && says("unsupported signature algorithm"));
      EXPECT(ks == nullptr);
    }
  }
  size_t info[4] = {7, 7, 7, 7};
  EXPECT(qrk_mldsa_keyset_info(nullptr, info) == -1 && says("null key set"));
  EXPECT(qrk_mldsa_keyset_info(nullptr, nullptr) == -1);
  EXPECT(info[0] == 7 && info[3] == 7);
  qrk_mldsa_keyset_free(nullptr);

  uint8_t buf[64] = {0};
  uint32_t index[2] = {0, 1};
  uint64_t off[3] = {0, 1, 2};
  int32_t status[2] = {7, 7};
  EXPECT(qrk_mldsa_verify_keyed_batch(nullptr, nullptr, 2, index, buf, off, buf, nullptr, 0, status, nullptr) == -1 &&
         says("null context"));
  EXPECT(qrk_mldsa_verify_keyed_batch(fake, nullptr, 2, index, buf, off, buf, nullptr, 0, status, nullptr) == -1 &&
         says("null key set"));
  EXPECT(qrk_mldsa_verify_keyed_batch(fake, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 256, nullptr,
                                      nullptr) == -1 && says("null key set"));
  EXPECT(qrk_mldsa_sign_keyed_batch(nullptr, nullptr, 2, index, buf, off, nullptr, nullptr, 0, buf, status, nullptr) ==
         -1 && says("null context"));
  EXPECT(qrk_mldsa_sign_keyed_batch(fake, nullptr, 2, index, buf, off, nullptr, buf, 255, buf, status, nullptr) == -1 &&
         says("null key set"));
  EXPECT(status[0] == 7 && status[1] == 7);

  // with a real context the loaders go on to the device: without one they fail there, cleanly
  qrk_ctx* ctx = nullptr;
  if (qrk_ctx_create(&ctx, 0) == 0) {
    qrk_mldsa_keyset* ks = nullptr;
    EXPECT(qrk_mldsa_verify_keyed_batch(ctx, nullptr, 1, index, buf, off, buf, nullptr, 0, status, nullptr) == -1 &&
           says("null key set"));
    EXPECT(qrk_mldsa_pubkeys_load(ctx, "ML-DSA-44", 0, keys, &ks, nullptr) == -1);
    qrk_ctx_destroy(ctx);
  } else {
    EXPECT(ctx == nullptr);
  }
  std::free(keys);
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
