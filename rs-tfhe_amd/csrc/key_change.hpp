// key_change.hpp -- the one path by which a key becomes current on a handle (host code only).
//
// Every route that changes a cloud key or a re-encryption key (load, generate, compressed load / generate, adopt, the
// pool's two replications, the re-encryption key that shares d_ksk) runs
//   begin_key_change:  drain what may still read the old key (drain_key_readers), clear key_loaded and reenc_loaded,
//                      allocate the buffers the route names (ensure_key_buffers)
//   ... the route fills the buffers on ctx->stream ...
//   commit_cloud_key / commit_reenc_key:  rebuild the matrix-core byte planes, set the offset, set the flag LAST,
//                      warm lane 0 of the front end
// and a route that leaves in between leaves both flags cleared: the handle answers "cloud key not loaded" until the
// next change succeeds.  The real differences between the routes, all of them kept:
//  - argument validation comes BEFORE begin_key_change, so a refused call leaves the old key answering;
//  - tfhe_hip_adopt_cloud_key is a commit with no begin: the caller filled the buffers (on streams of its own), so it
//    quiesces the lanes and synchronises the whole device first, and the old flag stands until the commit;
//  - the pool's broadcast replication splits begin (prepare_replica) and commit (finish_replica) around the
//    broadcast, which runs outside the member's call, and synchronises the whole device before the commit;
// The side keys -- the packing key (packing.hpp, packing_keygen.hpp), the public key (pk_encrypt.hpp) and the sixteen
// TRLWE switching keys (trlwe_switch.hpp: plain rows, one flag an entry) -- have their
// own flags and byte planes, which are not the key switch's, and their own, smaller pair: begin_side_key drains the
// whole device, clears the side key's flag and grows its planes; the route fills them; commit_side_key sets the flag
// LAST.  A cloud-key change leaves them alone, and validation comes before the begin here too.
// ctx->mu is held and ctx's device is current in everything below.
// Part of tfhe_hip.hip.  What the feature units use of it -- the begin / commit pairs, the staged secrets, the row
// launches -- is declared in internal.hpp, with the types and the sizes of the key buffers.
#pragma once

namespace {
// d_ksk is allocated this much longer: the key switch's row DMAs read past the end of the last row (key_switch.hpp)
constexpr size_t kKskTailPad = 4096;

// the only allocator of d_bsk / d_ksk / d_testvec (they go with their KeyState)
int ensure_key_buffers(tfhe_hip_ctx *ctx, int which) {
  KeyState &k = *ctx->K;
  if (which & KEY_BUF_BSK) CHK(alloc_exact(ctx, k.d_bsk, bsk_bytes(ctx->P), "hipMalloc((void **)&k.d_bsk, bsk_bytes(ctx->P))"));
  if (which & KEY_BUF_KSK) CHK(alloc_exact(ctx, k.d_ksk, ksk_bytes(ctx->P) + kKskTailPad, "hipMalloc((void **)&k.d_ksk, ksk_bytes(ctx->P) + kKskTailPad)"));
  if (which & KEY_BUF_TESTVEC) CHK(alloc_exact(ctx, k.d_testvec, key_testvec_bytes(), "hipMalloc((void **)&k.d_testvec, key_testvec_bytes())"));
  return TFHE_HIP_OK;
}

// Work queued earlier on a caller's stream (*_dev entry points), on the context's stream or on the front end's lanes
// (merged small calls) may still be reading the key that is about to change: drain all three.
// (The key-view branch of tfhe_hip_ctx_destroy keeps its own spelling: it must go on to free the key whatever a
// synchronisation answers, and this returns at the first failure.)
int drain_key_readers(tfhe_hip_ctx *ctx) {
  CHK(hip_rc(ctx, sync_scratch_owner(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->scratch.owned = false;
  comb_quiesce(ctx);
  return TFHE_HIP_OK;
}
}  // namespace

// `which`: KEY_BUF_ALL for a cloud key, KEY_BUF_KSK for a re-encryption key (d_ksk is shared between the two, hence
// both flags go)
int begin_key_change(tfhe_hip_ctx *ctx, int which) {
  CHK(drain_key_readers(ctx));
  ctx->K->key_loaded = ctx->K->reenc_loaded = false;
  return ensure_key_buffers(ctx, which);
}

int commit_cloud_key(tfhe_hip_ctx *ctx, uint32_t offset) {
  CHK(build_ksk_planes(ctx));
  ctx->K->offset = offset;
  ctx->K->reenc_loaded = false;  // (already so after begin_key_change; adopt has no begin)
  ctx->K->key_loaded = true;
  comb_prepare(ctx);
  return TFHE_HIP_OK;
}

int commit_reenc_key(tfhe_hip_ctx *ctx) {
  CHK(build_ksk_planes(ctx));
  ctx->K->reenc_loaded = true;
  return TFHE_HIP_OK;
}

// ---- side keys ------------------------------------------------------------------------------------------------------
// `flag` / `planes` are the side key's members of *ctx->K.  Calls queued on the caller's streams may still read
// the planes that are about to be overwritten: hence the device-wide drain.
int begin_side_key(tfhe_hip_ctx *ctx, bool &flag, DevBuf &planes, size_t bytes) {
  HIPCHK(ctx, hipDeviceSynchronize());
  flag = false;
  return alloc_exact(ctx, planes, bytes, "hipMalloc((void **)&planes, bytes)");
}

// The *_is_loaded calls: 0 / 1, never an error code, no device call.  No lock: the host mirrors ask this before EVERY
// call (is the view's key resident yet?), and the context's mutex may be held for the length of a 65,536-ciphertext
// host call -- a one-gate call on another thread would wait 330 ms just to learn what it already knows.  A flag is set
// last by the calls that load a key and cleared first by those that change one; a caller that races its own key load is
// the caller's to order (as for any call under that key).
int flag_is_loaded(tfhe_hip_ctx *ctx, bool KeyState::*flag) {
  if (!ctx) return 0;
  return __atomic_load_n(&(ctx->own.*flag), __ATOMIC_ACQUIRE) ? 1 : 0;
}

// ---- the key-switching key between its two layouts ---------------------------------------------------------------------
hipError_t ksk_convert_launch(tfhe_hip_ctx *ctx, const uint32_t *d_ref, size_t rows) {
  hipLaunchKernelGGL(k_ksk_convert, dim3((unsigned)rows), dim3(256), 0, ctx->stream, d_ref, ctx->K->d_ksk, ctx->P.n,
                     1 << ctx->P.basebit, rows);
  return hipGetLastError();
}
hipError_t ksk_export_launch(tfhe_hip_ctx *ctx, uint32_t *d_ref, size_t rows) {
  hipLaunchKernelGGL(k_ksk_export, dim3((unsigned)rows), dim3(256), 0, ctx->stream, ctx->K->d_ksk, d_ref, ctx->P.n, rows);
  return hipGetLastError();
}

namespace {
// the kernel's CSPRNG, as the reference's thread_rng is seeded (OsRng)
int os_random(uint8_t *buf, size_t bytes) {  // 0, or errno
  size_t got = 0;
  while (got < bytes) {
    const ssize_t r = getrandom(buf + got, bytes - got, 0);
    if (r < 0) {
      if (errno == EINTR) continue;
      return errno;
    }
    got += (size_t)r;
  }
  return 0;
}
std::string os_random_text(int err) { return std::string("getrandom: ") + strerror(err); }

}  // namespace

int GeneratorKey::fill(tfhe_hip_ctx *ctx, const uint8_t *rng_key) {
  if (rng_key) {
    memcpy(k.k, rng_key, 32);  // 8 little-endian words
  } else if (const int err = os_random((uint8_t *)k.k, sizeof(k.k))) {
    return fail(ctx, TFHE_HIP_EHIP, os_random_text(err));
  }
  return TFHE_HIP_OK;
}

// ---- key generation: the secrets on the device (StagedSecrets, internal.hpp) -------------------------------------------
int key_spectrum_launch(tfhe_hip_ctx *ctx, const uint32_t *d_key_lv1, double2 *d_spec, hipStream_t s) {
  hipLaunchKernelGGL(k_key_spectrum, dim3(1), dim3(64), kStageLdsBytes, s, d_key_lv1, ctx->d_tw, d_spec);
  return launched(ctx);
}

int stage_secrets(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, const ChaChaKey &rk, StagedSecrets &s) {
  const size_t k0_at = 2 * sizeof(ChaChaKey), k1_at = k0_at + s.k0_words * 4;
  const size_t spec_at = (k1_at + (size_t)kN * 4 + 15) & ~(size_t)15;
  s.stage.put(&rk, sizeof(ChaChaKey), 0);
  s.stage.put(key_lv0, s.k0_words * 4, k0_at);
  s.stage.put(key_lv1, (size_t)kN * 4, k1_at);
  CHK(s.stage.land("key generation: ", spec_at + (size_t)kN2 * sizeof(double2)));
  s.d_rk = s.stage.dev<ChaChaKey>(0);
  s.d_k0 = s.stage.dev(k0_at);
  s.d_k1 = s.stage.dev(k1_at);
  CHK(key_spectrum_launch(ctx, s.d_k1, s.stage.dev<double2>(spec_at), ctx->stream));
  s.d_spec = s.stage.dev<const double2>(spec_at);
  return TFHE_HIP_OK;
}

// (the seed streams of the library, instantiated below: every unit's k_derive_stream_seed is emitted here)
template <uint32_t STREAM>
int derive_public_seed(tfhe_hip_ctx *ctx, const StagedSecrets &s, ChaChaKey &seed) {
  hipLaunchKernelGGL((k_derive_stream_seed<64, STREAM>), dim3(1), dim3(64), 0, ctx->stream, s.d_rk, s.d_rk + 1);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(&seed, s.d_rk + 1, sizeof(seed), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_HIP_OK;
}
template int derive_public_seed<kStreamSeededSeed>(tfhe_hip_ctx *, const StagedSecrets &, ChaChaKey &);  // seeded.hpp
template int derive_public_seed<kStreamPackSeed>(tfhe_hip_ctx *, const StagedSecrets &, ChaChaKey &);    // packing_keygen.hpp
template int derive_public_seed<kStreamTksSeed>(tfhe_hip_ctx *, const StagedSecrets &, ChaChaKey &);     // trlwe_switch.hpp
template int derive_public_seed<kStreamTrgswSeed>(tfhe_hip_ctx *, const StagedSecrets &, ChaChaKey &);   // cmux.hpp

int lwe_rows_launch(tfhe_hip_ctx *ctx, const LweRowJob &j, hipStream_t s) {
  const tfhe_hip_params &P = ctx->P;
  if (P.n > kLweMaxN) return fail(ctx, TFHE_HIP_EINVAL, "n too large");  // (params_supported admits no such context)
  const size_t per = (size_t)kLweWaves * kLweRowsPerWave;
  const dim3 grid((unsigned)((j.rows + per - 1) / per)), wg(64 * kLweWaves);
  if (j.k) hipLaunchKernelGGL((k_lwe_rows<kLweWaves, false>), grid, wg, 0, s, j, P.n, P.basebit, P.t);
  else hipLaunchKernelGGL((k_lwe_rows<kLweWaves, true>), grid, wg, 0, s, j, P.n, P.basebit, P.t);
  return launched(ctx);
}

int ksk_rows_launch(tfhe_hip_ctx *ctx, const StagedSecrets &s, const ChaChaKey *seed, double alpha, uint32_t *bodies,
                    uint32_t *out) {
  LweRowJob j{};
  if (seed) j.seed = *seed;
  j.k = s.d_rk;
  j.mask_under_k = !seed;
  j.stream_mask = seed ? kStreamSeededKskMask : kStreamKskMask;
  j.stream_noise = seed ? kStreamSeededKskNoise : kStreamKskNoise;
  j.dom_mask = j.dom_noise = kSeedDomainKsk;
  j.rows = ksk_rows(ctx->P);
  j.alpha = alpha;
  j.s0 = s.d_k0;
  j.key_rows = true;
  j.key_from = s.d_k1;
  j.bodies = bodies;
  j.out = out;
  j.stride = ksk_row_words(ctx->P.n);
  return lwe_rows_launch(ctx, j, ctx->stream);
}

int default_offset_and_testvec(tfhe_hip_ctx *ctx, uint32_t *offset) {
  const tfhe_hip_params &P = ctx->P;
  uint32_t off = 0;
  for (int i = 0; i < P.l; ++i) off += ((1u << P.bgbit) / 2) * (1u << (32 - (i + 1) * P.bgbit));
  std::vector<uint32_t> tv(2 * kN, 0u);
  for (int i = 0; i < kN; ++i) tv[kN + i] = 0x20000000u;  // f64_to_torus(0.125)
  HIPCHK(ctx, hipMemcpyAsync(ctx->K->d_testvec, tv.data(), key_testvec_bytes(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (the local test vector above is read by an asynchronous copy)
  *offset = off;
  return TFHE_HIP_OK;
}
