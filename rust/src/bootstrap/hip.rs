// rust/src/bootstrap/hip.rs -- the crate-side binding of libtfhe_hip.so for thedonutfactory/rs-tfhe.
//
// Copy to `src/bootstrap/hip.rs` of the crate and add `#[cfg(feature = "hip")] pub mod hip;` to `src/bootstrap/mod.rs`.
// UNCOMPILED: the image this repository is built in has no Rust toolchain.  What holds it to the C ABI meanwhile is
// tests/test_binding_lint.py (every `extern "C"` declaration below against include/tfhe_hip.h: arity, pointer depth,
// constness, integer widths, return type, and the symbol exported by the built library); the same API surface is
// compiled and run on the GPU through the C++ mirror include/rs_tfhe_hip.hpp (tests/cpp/test_mirror.cpp).
// Interfaces bound: src/bootstrap/mod.rs:23-43 (trait Bootstrap: Send + Sync), src/gates.rs:43-45, src/trgsw.rs:53-55;
// FFI precedent in the reference itself: src/fft/spqlios/spqlios_fft.rs:23-34.
//! MI355X bootstrap strategies: blind rotate + sample extract + key switch on the GPU(s).
use crate::bootstrap::Bootstrap;
use crate::key::CloudKey;
#[cfg(feature = "lut-bootstrap")]
use crate::lut::LookupTable;
use crate::{params, trlwe};
use crate::utils::Ciphertext;
use std::cell::RefCell;
use std::os::raw::{c_char, c_int, c_void};
use std::sync::Mutex;

#[repr(C)]
struct TfheHipParams { n: i32, l: i32, bgbit: i32, basebit: i32, t: i32 }
#[repr(C)]
pub struct TfheHipPool { _private: [u8; 0] }

extern "C" {   // include/tfhe_hip.h, the tfhe_hip_pool_* family: one handle, 1..64 devices
    fn tfhe_hip_device_count() -> c_int;
    fn tfhe_hip_pool_create(p: *const TfheHipParams, devices: *const c_int, ndev: c_int,
                            out: *mut *mut TfheHipPool) -> c_int;
    fn tfhe_hip_pool_key_create(pool: *mut TfheHipPool, key_view: *mut *mut TfheHipPool) -> c_int;  // another resident key
    fn tfhe_hip_pool_destroy(pool: *mut TfheHipPool);   // a pool, or a key view of one (views first)
    fn tfhe_hip_pool_last_error(pool: *const TfheHipPool) -> *const c_char;
    fn tfhe_hip_pool_load_cloud_key(pool: *mut TfheHipPool, bsk: *const f64, ksk: *const u32,
                                    decomp_offset: u32, testvec: *const u32) -> c_int;
    fn tfhe_hip_pool_gen_cloud_key_with_key(pool: *mut TfheHipPool, key_lv0: *const u32, key_lv1: *const u32,
                                            alpha_ksk: f64, alpha_bsk: f64, rng_key: *const u8) -> c_int;
    fn tfhe_hip_pool_export_cloud_key(pool: *mut TfheHipPool, member: c_int, bsk: *mut f64, ksk: *mut u32,
                                      decomp_offset: *mut u32, testvec: *mut u32) -> c_int;
    fn tfhe_hip_pool_batch_gate(pool: *mut TfheHipPool, gate: c_int, a: *const u32, b: *const u32,
                                out: *mut u32, count: usize) -> c_int;
    fn tfhe_hip_pool_batch_gates_mixed(pool: *mut TfheHipPool, gates: *const u8, a: *const u32, b: *const u32,
                                       out: *mut u32, count: usize) -> c_int;
    fn tfhe_hip_pool_batch_bootstrap(pool: *mut TfheHipPool, input: *const u32, testvec: *const u32,
                                     per_ct: c_int, keyswitch: c_int, out: *mut u32, count: usize) -> c_int;
    fn tfhe_hip_pool_batch_blind_rotate(pool: *mut TfheHipPool, input: *const u32, testvec: *const u32,
                                        out_trlwe: *mut u32, count: usize) -> c_int;
    fn tfhe_hip_pool_batch_mux(pool: *mut TfheHipPool, naive: c_int, a: *const u32, b: *const u32,
                               c: *const u32, out: *mut u32, count: usize) -> c_int;
    // a batch RESIDENT on one member's GPU: device pointers, shards travel by grouped RCCL send / receive (or peer copies)
    fn tfhe_hip_pool_batch_gate_dev(pool: *mut TfheHipPool, home_member: c_int, gate: c_int, a: *const u32,
                                    b: *const u32, out: *mut u32, count: usize, stream: *mut c_void) -> c_int;
    fn tfhe_hip_pool_batch_gates_mixed_dev(pool: *mut TfheHipPool, home_member: c_int, gates: *const u8, a: *const u32,
                                           b: *const u32, out: *mut u32, count: usize, stream: *mut c_void) -> c_int;
    fn tfhe_hip_pool_batch_gates_mixed_nks_dev(pool: *mut TfheHipPool, home_member: c_int, gates: *const u8,
                                               a: *const u32, b: *const u32, out: *mut u32, count: usize,
                                               stream: *mut c_void) -> c_int;
    fn tfhe_hip_pool_batch_bootstrap_dev(pool: *mut TfheHipPool, home_member: c_int, input: *const u32,
                                         testvec: *const u32, per_ct: c_int, keyswitch: c_int, out: *mut u32,
                                         count: usize, stream: *mut c_void) -> c_int;
    fn tfhe_hip_pool_batch_lincomb_bootstrap_dev(pool: *mut TfheHipPool, home_member: c_int, ca: u32, a: *const u32,
                                                 cb: u32, b: *const u32, cconst: u32, testvec: *const u32,
                                                 per_ct: c_int, keyswitch: c_int, out: *mut u32, count: usize,
                                                 stream: *mut c_void) -> c_int;
    // many-LUT bootstrap: n_luts functions packed in one test vector from one blind rotation, out [n_luts][count][n+1]
    fn tfhe_hip_pool_batch_lincomb_bootstrap_many(pool: *mut TfheHipPool, ca: u32, a: *const u32, cb: u32,
                                                  b: *const u32, cconst: u32, testvec: *const u32, per_ct: c_int,
                                                  n_luts: c_int, keyswitch: c_int, out: *mut u32, count: usize) -> c_int;
    fn tfhe_hip_pool_batch_lincomb_bootstrap_many_dev(pool: *mut TfheHipPool, home_member: c_int, ca: u32,
                                                      a: *const u32, cb: u32, b: *const u32, cconst: u32,
                                                      testvec: *const u32, per_ct: c_int, n_luts: c_int,
                                                      keyswitch: c_int, out: *mut u32, count: usize,
                                                      stream: *mut c_void) -> c_int;
    fn tfhe_hip_pool_batch_mux_dev(pool: *mut TfheHipPool, home_member: c_int, naive: c_int, a: *const u32,
                                   b: *const u32, c: *const u32, out: *mut u32, count: usize,
                                   stream: *mut c_void) -> c_int;
    // seeded (compressed) cloud key: the bodies travel, the masks are regenerated from the public seed on the device
    fn tfhe_hip_pool_load_compressed_cloud_key(pool: *mut TfheHipPool, mask_seed: *const u8, bsk_bodies: *const u32,
                                               ksk_bodies: *const u32, decomp_offset: u32, testvec: *const u32) -> c_int;
    fn tfhe_hip_pool_synchronize(pool: *mut TfheHipPool) -> c_int;
    fn tfhe_hip_pool_data_transport(pool: *const TfheHipPool) -> *const c_char;
    fn tfhe_hip_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;   // pinned host memory
    fn tfhe_hip_host_free(p: *mut c_void);
}

pub const NAND: c_int = 0; pub const OR: c_int = 1; pub const AND: c_int = 2; pub const XOR: c_int = 3;
pub const XNOR: c_int = 4; pub const NOR: c_int = 5; pub const ANDNY: c_int = 6; pub const ANDYN: c_int = 7;
pub const ORNY: c_int = 8; pub const ORYN: c_int = 9; pub const COPY: c_int = 10;

extern "C" {   // packing key switch (include/tfhe_hip.h): up to N lv0 results in one TRLWE lv1 under the client's s1
    fn tfhe_hip_pool_load_packing_key(pool: *mut TfheHipPool, mask_seed: *const u8, bodies: *const u32) -> c_int;
    // the packing key generated on the first member's GPU (a client-side call: it takes the secret key); bodies may be null
    fn tfhe_hip_pool_gen_packing_key(pool: *mut TfheHipPool, key_lv0: *const u32, key_lv1: *const u32, alpha: f64,
                                     rng_key: *const u8, mask_seed: *mut u8, bodies: *mut u32) -> c_int;
    fn tfhe_hip_pool_batch_pack_tlwe(pool: *mut TfheHipPool, input: *const u32, count: usize, out: *mut u32) -> c_int;
    // unpacking key switch: slots of TRLWE lv1 ciphertexts back to lv0 ciphertexts under the cloud key's key-switching key
    fn tfhe_hip_pool_batch_unpack_trlwe(pool: *mut TfheHipPool, trlwe: *const u32, groups: usize, slots: *const u32,
                                        count: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_pool_batch_unpack_trlwe_dev(pool: *mut TfheHipPool, home_member: c_int, trlwe: *const u32, groups: usize,
                                            slots: *const u32, count: usize, out: *mut u32, stream: *mut c_void) -> c_int;
    // encrypted-table key switch and the tree bootstrap: any function of two encrypted digits.  pack_table has no pool
    // form: it runs on a member context (tfhe_hip_pool_ctx) of the packing key's view
    fn tfhe_hip_pool_ctx(pool: *mut TfheHipPool, member: c_int) -> *mut TfheHipCtx;
    fn tfhe_hip_last_error(ctx: *const TfheHipCtx) -> *const c_char;
    fn tfhe_hip_batch_pack_table(ctx: *mut TfheHipCtx, input: *const u32, m: c_int, count: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_pool_batch_bootstrap_bivariate(pool: *mut TfheHipPool, x: *const u32, y: *const u32, testvecs: *const u32,
                                               m: c_int, n_luts: c_int, keyswitch: c_int, out: *mut u32,
                                               count: usize) -> c_int;
    // public-key encryption and the asymmetric re-encryption key (include/tfhe_hip.h): no pool forms, they run on a
    // member context (tfhe_hip_pool_ctx) of the public key's view
    fn tfhe_hip_load_public_key(ctx_or_view: *mut TfheHipCtx, encryptions: *const u32, size: usize) -> c_int;
    fn tfhe_hip_batch_pk_encrypt(ctx: *mut TfheHipCtx, plain: *const u32, count: usize, alpha: f64, rng_key: *const u8,
                                 first_index: u64, out: *mut u32) -> c_int;
    fn tfhe_hip_gen_reenc_key_asymmetric(ctx_or_view: *mut TfheHipCtx, key_from: *const u32, alpha: f64,
                                         rng_key: *const u8, key_out: *mut u32) -> c_int;
    fn tfhe_hip_batch_reencrypt(ctx: *mut TfheHipCtx, input: *const u32, out: *mut u32, count: usize) -> c_int;
    // symmetric encryption (include/tfhe_hip.h): bulk ciphertexts, the public key and the symmetric re-encryption key
    // made on the device; no pool forms either
    fn tfhe_hip_batch_encrypt(ctx: *mut TfheHipCtx, key_lv0: *const u32, plain: *const u32, count: usize, alpha: f64,
                              rng_key: *const u8, mask_seed: *const u8, first_index: u64, bodies: *mut u32,
                              out: *mut u32) -> c_int;
    fn tfhe_hip_gen_public_key(ctx_or_view: *mut TfheHipCtx, key_lv0: *const u32, size: usize, alpha: f64,
                               rng_key: *const u8, encryptions_out: *mut u32) -> c_int;
    fn tfhe_hip_gen_reenc_key_symmetric(ctx_or_view: *mut TfheHipCtx, key_from: *const u32, key_to: *const u32,
                                        alpha: f64, rng_key: *const u8, key_out: *mut u32) -> c_int;
    // decryption (include/tfhe_hip.h): phases, booleans and messages of LWE rows and of packed TRLWE slots; no pool forms
    fn tfhe_hip_batch_decrypt(ctx: *mut TfheHipCtx, key: *const u32, key_len: usize, input: *const u32, count: usize,
                              mode: c_int, modulus: u32, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_decrypt_dev(ctx: *mut TfheHipCtx, key: *const u32, key_len: usize, input: *const u32, count: usize,
                                  mode: c_int, modulus: u32, out: *mut u32, stream: *mut c_void) -> c_int;
    fn tfhe_hip_batch_decrypt_trlwe(ctx: *mut TfheHipCtx, key_lv1: *const u32, trlwe: *const u32, groups: usize,
                                    count: usize, mode: c_int, modulus: u32, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_decrypt_trlwe_dev(ctx: *mut TfheHipCtx, key_lv1: *const u32, trlwe: *const u32, groups: usize,
                                        count: usize, mode: c_int, modulus: u32, out: *mut u32,
                                        stream: *mut c_void) -> c_int;
    // packed encryption (include/tfhe_hip.h): TRLWE lv1 ciphertexts, N values each -- full, seeded and expansion; no pool forms
    fn tfhe_hip_batch_encrypt_trlwe(ctx: *mut TfheHipCtx, key_lv1: *const u32, plain: *const u32, count: usize, alpha: f64,
                                    rng_key: *const u8, mask_seed: *const u8, first_group: u64, bodies: *mut u32,
                                    out: *mut u32) -> c_int;
    fn tfhe_hip_batch_encrypt_trlwe_dev(ctx: *mut TfheHipCtx, key_lv1: *const u32, plain: *const u32, count: usize,
                                        alpha: f64, rng_key: *const u8, mask_seed: *const u8, first_group: u64,
                                        bodies: *mut u32, out: *mut u32, stream: *mut c_void) -> c_int;
    fn tfhe_hip_expand_seeded_trlwe(ctx: *mut TfheHipCtx, mask_seed: *const u8, first_group: u64, bodies: *const u32,
                                    groups: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_expand_seeded_trlwe_dev(ctx: *mut TfheHipCtx, mask_seed: *const u8, first_group: u64, bodies: *const u32,
                                        groups: usize, out: *mut u32, stream: *mut c_void) -> c_int;
    // TRLWE key switch (include/tfhe_hip.h): packed re-encryption (k = 1) and slot automorphisms; no pool forms
    fn tfhe_hip_trlwe_switch_key_words(t: c_int, body_words: *mut usize) -> c_int;
    fn tfhe_hip_gen_trlwe_switch_key(ctx: *mut TfheHipCtx, key_from_lv1: *const u32, key_to_lv1: *const u32, k: c_int,
                                     basebit: c_int, t: c_int, alpha: f64, rng_key: *const u8, mask_seed: *mut u8,
                                     bodies: *mut u32) -> c_int;
    fn tfhe_hip_load_trlwe_switch_key(ctx: *mut TfheHipCtx, k: c_int, basebit: c_int, t: c_int, mask_seed: *const u8,
                                      bodies: *const u32) -> c_int;
    fn tfhe_hip_batch_trlwe_keyswitch(ctx: *mut TfheHipCtx, k: c_int, input: *const u32, count: usize, out: *mut u32) -> c_int;
    // packed CMUX (include/tfhe_hip.h): caller-held TRGSW selectors; no key, no pool forms
    fn tfhe_hip_batch_trlwe_cmux(ctx: *mut TfheHipCtx, sel: *const u32, basebit: c_int, t: c_int, flags: c_int, d0: *const u32,
                                 d1: *const u32, count: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_encrypt_trgsw(ctx: *mut TfheHipCtx, key_lv1: *const u32, mu: *const int32_t, count: usize, basebit: c_int,
                                    t: c_int, alpha: f64, rng_key: *const u8, first_index: u64, mask_seed_out: *mut u8,
                                    out: *mut u32) -> c_int;
}

/// TFHE_HIP_CMUX_REFERENCE_DIGITS: the reference's truncating decomposition (trgsw.rs:144-171) in `HipEngine::trlwe_cmux`
pub const CMUX_REFERENCE_DIGITS: c_int = 1;

/// TFHE_HIP_DECRYPT_*: what `HipEngine::decrypt_batch` and `decrypt_trlwe` return per ciphertext
pub const DECRYPT_PHASE: c_int = 0;     // b - <a, s>, wrapping u32
pub const DECRYPT_BOOL: c_int = 1;      // 1 where the phase read as i32 is >= 0 (TLWELv0::decrypt_bool), else 0
pub const DECRYPT_MESSAGE: c_int = 2;   // TLWELv0::decrypt_lwe_message mod `modulus`, 2 <= modulus <= 65536

#[allow(non_camel_case_types)]
type int8_t = i8;   // the header's spelling of the weights' type
#[allow(non_camel_case_types)]
type int32_t = i32;   // ... and of a selector's message coefficients

extern "C" {   // encrypted linear layers (include/tfhe_hip.h): a plaintext int8 matrix times LWE ciphertexts or TRLWE slots;
    // no pool forms, they run on a member context (tfhe_hip_pool_ctx) of the cloud key's view
    fn tfhe_hip_batch_tlwe_matmul(ctx: *mut TfheHipCtx, w: *const int8_t, bias: *const u32, rows: usize, cols: usize,
                                  input: *const u32, groups: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_tlwe_matmul_dev(ctx: *mut TfheHipCtx, w: *const int8_t, bias: *const u32, rows: usize, cols: usize,
                                      input: *const u32, groups: usize, out: *mut u32, stream: *mut c_void) -> c_int;
    fn tfhe_hip_batch_trlwe_matmul(ctx: *mut TfheHipCtx, w: *const int8_t, bias: *const u32, rows: usize, cols: usize,
                                   trlwe: *const u32, groups: usize, keyswitch: c_int, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_trlwe_matmul_dev(ctx: *mut TfheHipCtx, w: *const int8_t, bias: *const u32, rows: usize, cols: usize,
                                       trlwe: *const u32, groups: usize, keyswitch: c_int, out: *mut u32,
                                       stream: *mut c_void) -> c_int;
    // plaintext polynomial products on packed ciphertexts (include/tfhe_hip.h): TRLWE in, TRLWE out
    fn tfhe_hip_batch_trlwe_polymul(ctx: *mut TfheHipCtx, w: *const int8_t, bias: *const u32, rows: usize, cols: usize,
                                    trlwe: *const u32, groups: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_trlwe_polymul_dev(ctx: *mut TfheHipCtx, w: *const int8_t, bias: *const u32, rows: usize, cols: usize,
                                        trlwe: *const u32, groups: usize, out: *mut u32, stream: *mut c_void) -> c_int;
    // encrypted 2-D convolution (include/tfhe_hip.h): int8 filters over a channels-last map of LWE ciphertexts
    fn tfhe_hip_batch_tlwe_conv2d(ctx: *mut TfheHipCtx, shape: *const TfheHipConv2dShape, w: *const int8_t, bias: *const u32,
                                  input: *const u32, groups: usize, out: *mut u32) -> c_int;
    fn tfhe_hip_batch_tlwe_conv2d_dev(ctx: *mut TfheHipCtx, shape: *const TfheHipConv2dShape, w: *const int8_t,
                                      bias: *const u32, input: *const u32, groups: usize, out: *mut u32,
                                      stream: *mut c_void) -> c_int;
}

/// `tfhe_hip_conv2d_shape`: the geometry of a 2-D convolution (include/tfhe_hip.h).  Strides are at least 1; the padding
/// is zeros on both sides of each axis.
#[derive(Clone, Copy, Debug)]
#[repr(C)]
pub struct TfheHipConv2dShape {
    pub in_h: u32,
    pub in_w: u32,
    pub in_c: u32,
    pub out_c: u32,
    pub k_h: u32,
    pub k_w: u32,
    pub stride_h: u32,
    pub stride_w: u32,
    pub pad_h: u32,
    pub pad_w: u32,
}
impl TfheHipConv2dShape {
    /// (out_h, out_w) = ((in_h + 2 pad_h - k_h) / stride_h + 1, likewise); the filter must fit the padded map.
    pub fn out_hw(&self) -> (usize, usize) {
        let (ph, pw) = (self.in_h as usize + 2 * self.pad_h as usize, self.in_w as usize + 2 * self.pad_w as usize);
        assert!(self.stride_h > 0 && self.stride_w > 0, "stride is at least 1");
        assert!(self.k_h > 0 && self.k_w > 0 && self.k_h as usize <= ph && self.k_w as usize <= pw, "the filter fits the padded map");
        ((ph - self.k_h as usize) / self.stride_h as usize + 1, (pw - self.k_w as usize) / self.stride_w as usize + 1)
    }
}

/// A member context of a pool (tfhe_hip_pool_ctx): opaque, owned by the pool.
#[repr(C)]
pub struct TfheHipCtx { _private: [u8; 0] }

const W: usize = params::tlwe_lv0::N + 1;     // words per TLWELv0
const N: usize = params::trgsw_lv1::N;        // 1024
const MAX_RESIDENT_KEYS: usize = 4;           // key views kept per pool (172 MB + 104 MB of byte planes each)

/// Grow-only pinned buffer (tfhe_hip_host_alloc): operands flattened into it are read / written in place by the GPU.
struct Pinned { p: *mut u32, words: usize }
impl Pinned {
    const fn new() -> Self { Pinned { p: std::ptr::null_mut(), words: 0 } }
    fn get(&mut self, words: usize) -> &mut [u32] {
        if words > self.words {
            unsafe { if !self.p.is_null() { tfhe_hip_host_free(self.p as *mut c_void); } }
            let mut q: *mut c_void = std::ptr::null_mut();
            let want = words + words / 4;
            assert_eq!(unsafe { tfhe_hip_host_alloc(want * 4, &mut q) }, 0, "tfhe_hip_host_alloc failed");
            self.p = q as *mut u32; self.words = want;
        }
        unsafe { std::slice::from_raw_parts_mut(self.p, words) }
    }
}
impl Drop for Pinned { fn drop(&mut self) { unsafe { if !self.p.is_null() { tfhe_hip_host_free(self.p as *mut c_void); } } } }
thread_local! {   // one arena per calling thread: a, b, c operands and the result
    static ARENA: RefCell<[Pinned; 4]> = RefCell::new([Pinned::new(), Pinned::new(), Pinned::new(), Pinned::new()]);
}

/// A resident key: (address, content sample) of the CloudKey it holds + its key view of the pool.
/// pk_fp: content sample of the packing key loaded beside the cloud key (bootstrap_bivariate), 0 = none.
struct KeyView { addr: usize, fp: u64, view: *mut TfheHipPool, last_use: u64, users: usize, pk_fp: u64 }

/// The resident packing key: (content sample of the key it holds, its key view of the pool; null until first use).
struct PackingView { fp: u64, view: *mut TfheHipPool }

/// Owns the C pool (one context per device) and the key views on it.
pub struct HipEngine { pool: *mut TfheHipPool, views: Mutex<(Vec<KeyView>, u64)>, packing: Mutex<PackingView>,
                       public_key: Mutex<PackingView> }   // (the public key's own view; `fp` is its size, 0 = none)
unsafe impl Send for HipEngine {}   // the library merges concurrent small calls into shared launches and serialises the rest per context; `views` is behind its Mutex
unsafe impl Sync for HipEngine {}

impl HipEngine {
    /// `devices`: HIP device indices, e.g. `&[0]` or `&[0, 1, 2, 3, 4, 5, 6, 7]` (all GPUs of a node).  Batch
    /// calls split their slice contiguously over the devices, exactly as `par_iter().map().collect()`
    /// (src/parallel/rayon_impl.rs:40-47) keeps input order.
    pub fn new(devices: &[i32]) -> Self {
        let p = TfheHipParams {
            n: params::tlwe_lv0::N as i32, l: params::trgsw_lv1::L as i32,
            bgbit: params::trgsw_lv1::BGBIT as i32, basebit: params::trgsw_lv1::BASEBIT as i32,
            t: params::trgsw_lv1::IKS_T as i32,
        };
        let mut pool = std::ptr::null_mut();
        let rc = unsafe { tfhe_hip_pool_create(&p, devices.as_ptr(), devices.len() as c_int, &mut pool) };
        assert_eq!(rc, 0, "tfhe_hip_pool_create failed");   // the reference has no Result on this path
        HipEngine { pool, views: Mutex::new((Vec::new(), 0)),
                    packing: Mutex::new(PackingView { fp: 0, view: std::ptr::null_mut() }),
                    public_key: Mutex::new(PackingView { fp: 0, view: std::ptr::null_mut() }) }
    }

    fn check(h: *mut TfheHipPool, rc: c_int) {
        if rc != 0 {
            let msg = unsafe { std::ffi::CStr::from_ptr(tfhe_hip_pool_last_error(h)) };
            panic!("tfhe_hip: {}", msg.to_string_lossy());
        }
    }

    /// a content sample of both keys + sizes (FNV-style mix), as the C++ mirror takes one
    fn fingerprint(ck: &CloudKey) -> u64 {
        let mut h: u64 = 0x9E37_79B9_7F4A_7C15 ^ ck.decomposition_offset as u64;
        let mut mix = |v: u64| { h = (h ^ v).wrapping_mul(0x0000_0100_0000_01B3); };
        let nk = ck.key_switching_key.len();
        for i in 0..64 { let t = &ck.key_switching_key[(nk - 1) - (nk - 1) * i / 64]; mix(t.p[i % W] as u64); }
        let nb = ck.bootstrapping_key.len();
        for i in 0..64 { let row = &ck.bootstrapping_key[(nb - 1) * i / 64].rows()[0]; mix(row.b[i].to_bits()); }
        mix(nk as u64); mix(nb as u64);
        h
    }

    /// CloudKey is not #[repr(C)] and TRGSWLv1FFT's field is private (src/trgsw.rs:53-55): marshal
    /// field by field into the flat layouts of tfhe_hip.h.  Needs one accessor in trgsw.rs:
    ///     impl TRGSWLv1FFT { pub fn rows(&self) -> &[trlwe::TRLWELv1FFT; L * 2] { &self.trlwe_fft } }
    fn upload(view: *mut TfheHipPool, ck: &CloudKey) {
        let mut bsk: Vec<f64> = Vec::with_capacity(ck.bootstrapping_key.len() * 2 * params::trgsw_lv1::L * 2 * N);
        for trgsw in ck.bootstrapping_key.iter() {
            for row in trgsw.rows().iter() { bsk.extend_from_slice(&row.a); bsk.extend_from_slice(&row.b); }
        }
        let mut ksk: Vec<u32> = Vec::with_capacity(ck.key_switching_key.len() * W);
        for t in ck.key_switching_key.iter() { ksk.extend_from_slice(&t.p); }
        let mut tv: Vec<u32> = Vec::with_capacity(2 * N);
        tv.extend_from_slice(&ck.blind_rotate_testvec.a);
        tv.extend_from_slice(&ck.blind_rotate_testvec.b);
        // uploaded to the first device once, replicated to the others device to device
        Self::check(view, unsafe { tfhe_hip_pool_load_cloud_key(view, bsk.as_ptr(), ksk.as_ptr(),
                                                                ck.decomposition_offset, tv.as_ptr()) });
    }

    /// Run `call(view)` under the key view of `ck`: found by (address, fingerprint), else created (dropping the least
    /// recently used IDLE view beyond MAX_RESIDENT_KEYS) and loaded.  The registry lock covers lookup / creation /
    /// upload only; the batch call itself runs outside it (the library serialises per context), so threads with
    /// different keys do not queue behind one another's 330 ms batches at this level.
    fn with_key<R>(&self, ck: &CloudKey, call: impl FnOnce(*mut TfheHipPool) -> (c_int, R)) -> R {
        let (addr, fp) = (ck as *const CloudKey as usize, Self::fingerprint(ck));
        let view = {
            let mut g = self.views.lock().unwrap();
            g.1 += 1;
            let tick = g.1;
            let views = &mut g.0;
            let idx = match views.iter().position(|v| v.addr == addr && v.fp == fp) {
                Some(i) => i,
                None => {
                    while views.len() >= MAX_RESIDENT_KEYS {
                        match views.iter().enumerate().filter(|(_, v)| v.users == 0).min_by_key(|(_, v)| v.last_use) {
                            Some((i, _)) => { unsafe { tfhe_hip_pool_destroy(views[i].view) }; views.remove(i); }
                            None => break,   // every view is in use: exceed the cap for now
                        }
                    }
                    let mut v = std::ptr::null_mut();
                    assert_eq!(unsafe { tfhe_hip_pool_key_create(self.pool, &mut v) }, 0, "tfhe_hip_pool_key_create failed");
                    Self::upload(v, ck);   // under the registry lock: a second thread with the same new key waits here
                    views.push(KeyView { addr, fp, view: v, last_use: 0, users: 0, pk_fp: 0 });
                    views.len() - 1
                }
            };
            views[idx].users += 1;
            views[idx].last_use = tick;
            views[idx].view
        };
        let (rc, r) = call(view);
        { let mut g = self.views.lock().unwrap(); if let Some(v) = g.0.iter_mut().find(|v| v.view == view) { v.users -= 1; } }
        Self::check(view, rc);
        r
    }

    /// flatten ciphertexts into pinned arena slot `slot`; the slice stays valid until the thread's next call
    fn flatten_into<'a>(arena: &'a mut [Pinned; 4], slot: usize, cts: impl Iterator<Item = impl std::borrow::Borrow<Ciphertext>>, n: usize) -> *const u32 {
        let buf = arena[slot].get(n * W);
        for (i, c) in cts.enumerate() { buf[i * W..(i + 1) * W].copy_from_slice(&c.borrow().p); }
        buf.as_ptr()
    }
    fn unflatten(flat: &[u32]) -> Vec<Ciphertext> {
        flat.chunks_exact(W).map(|c| { let mut t = Ciphertext::new(); t.p.copy_from_slice(c); t }).collect()
    }

    /// gates::batch_* (src/gates.rs:352-547): prep + blind rotate + extract + key switch, all devices
    pub fn batch_gate(&self, gate: c_int, inputs: &[(Ciphertext, Ciphertext)], ck: &CloudKey) -> Vec<Ciphertext> {
        ARENA.with(|ar| {
            let ar = &mut *ar.borrow_mut();
            let a = Self::flatten_into(ar, 0, inputs.iter().map(|p| &p.0), inputs.len());
            let b = Self::flatten_into(ar, 1, inputs.iter().map(|p| &p.1), inputs.len());
            let out = ar[3].get(inputs.len() * W).as_mut_ptr();
            self.with_key(ck, |v| (unsafe { tfhe_hip_pool_batch_gate(v, gate, a, b, out, inputs.len()) }, ()));
            Self::unflatten(unsafe { std::slice::from_raw_parts(out, inputs.len() * W) })
        })
    }

    /// one launch per circuit level, one gate code per ciphertext (examples/add_two_numbers.rs)
    pub fn batch_gates_mixed(&self, gates: &[u8], inputs: &[(Ciphertext, Ciphertext)], ck: &CloudKey) -> Vec<Ciphertext> {
        assert_eq!(gates.len(), inputs.len());
        ARENA.with(|ar| {
            let ar = &mut *ar.borrow_mut();
            let a = Self::flatten_into(ar, 0, inputs.iter().map(|p| &p.0), inputs.len());
            let b = Self::flatten_into(ar, 1, inputs.iter().map(|p| &p.1), inputs.len());
            let out = ar[3].get(inputs.len() * W).as_mut_ptr();
            self.with_key(ck, |v| (unsafe { tfhe_hip_pool_batch_gates_mixed(v, gates.as_ptr(), a, b, out, inputs.len()) }, ()));
            Self::unflatten(unsafe { std::slice::from_raw_parts(out, inputs.len() * W) })
        })
    }

    /// Bootstrap::bootstrap / bootstrap_without_key_switch / LutBootstrap::bootstrap_lut over a batch
    pub fn batch_bootstrap(&self, cts: &[Ciphertext], testvec: Option<&trlwe::TRLWELv1>, keyswitch: bool, ck: &CloudKey) -> Vec<Ciphertext> {
        let tv: Option<Vec<u32>> = testvec.map(|t| { let mut v = Vec::with_capacity(2 * N); v.extend_from_slice(&t.a); v.extend_from_slice(&t.b); v });
        let tvp = tv.as_ref().map_or(std::ptr::null(), |v| v.as_ptr());
        ARENA.with(|ar| {
            let ar = &mut *ar.borrow_mut();
            let a = Self::flatten_into(ar, 0, cts.iter(), cts.len());
            let out = ar[3].get(cts.len() * W).as_mut_ptr();
            self.with_key(ck, |v| (unsafe { tfhe_hip_pool_batch_bootstrap(v, a, tvp, 0, keyswitch as c_int, out, cts.len()) }, ()));
            Self::unflatten(unsafe { std::slice::from_raw_parts(out, cts.len() * W) })
        })
    }

    /// trgsw::batch_blind_rotate (src/trgsw.rs:289-294)
    pub fn batch_blind_rotate(&self, srcs: &[Ciphertext], ck: &CloudKey) -> Vec<trlwe::TRLWELv1> {
        ARENA.with(|ar| {
            let ar = &mut *ar.borrow_mut();
            let a = Self::flatten_into(ar, 0, srcs.iter(), srcs.len());
            let mut out = vec![0u32; srcs.len() * 2 * N];   // 8 KiB per sample: staged by the library
            self.with_key(ck, |v| (unsafe { tfhe_hip_pool_batch_blind_rotate(v, a, std::ptr::null(), out.as_mut_ptr(), srcs.len()) }, ()));
            out.chunks_exact(2 * N).map(|c| { let mut t = trlwe::TRLWELv1::new(); t.a.copy_from_slice(&c[..N]); t.b.copy_from_slice(&c[N..]); t }).collect()
        })
    }

    /// Gates::mux (the reference's formula, gates.rs:157-183) / Gates::mux_naive (:189-199) over a batch
    pub fn batch_mux(&self, naive: bool, abc: &[(Ciphertext, Ciphertext, Ciphertext)], ck: &CloudKey) -> Vec<Ciphertext> {
        ARENA.with(|ar| {
            let ar = &mut *ar.borrow_mut();
            let a = Self::flatten_into(ar, 0, abc.iter().map(|t| &t.0), abc.len());
            let b = Self::flatten_into(ar, 1, abc.iter().map(|t| &t.1), abc.len());
            let c = Self::flatten_into(ar, 2, abc.iter().map(|t| &t.2), abc.len());
            let out = ar[3].get(abc.len() * W).as_mut_ptr();
            self.with_key(ck, |v| (unsafe { tfhe_hip_pool_batch_mux(v, naive as c_int, a, b, c, out, abc.len()) }, ()));
            Self::unflatten(unsafe { std::slice::from_raw_parts(out, abc.len() * W) })
        })
    }

    /// The same map for a batch that is ALREADY RESIDENT on member `home`'s GPU (the levels of a circuit, the output of a
    /// previous call): `a`, `b`, `out` are device pointers to `count` rows of n + 1 words on that GPU, `stream` a
    /// hipStream_t of it (null = the member's own).  The library cuts the batch over the members, moves the shards by
    /// grouped RCCL send / receive over its persistent communicator (peer copies when the pool repeats a device),
    /// bootstraps them in parallel and orders the gathered result into `stream`; the call only enqueues.
    /// Safety: the pointers must stay valid until the work has run (`synchronize`).
    pub unsafe fn batch_gate_dev(&self, home: usize, gate: c_int, a: *const u32, b: *const u32, out: *mut u32,
                                 count: usize, stream: *mut c_void, ck: &CloudKey) {
        self.with_key(ck, |v| (tfhe_hip_pool_batch_gate_dev(v, home as c_int, gate, a, b, out, count, stream), ()));
    }
    /// One circuit level on the device: per-ciphertext gate codes (device pointer), with or without the key switch
    /// (`keyswitch = false` is the first level of Gates::mux, gates.rs:165-177).
    pub unsafe fn batch_gates_mixed_dev(&self, home: usize, gates: *const u8, a: *const u32, b: *const u32, out: *mut u32,
                                        count: usize, keyswitch: bool, stream: *mut c_void, ck: &CloudKey) {
        self.with_key(ck, |v| (if keyswitch { tfhe_hip_pool_batch_gates_mixed_dev(v, home as c_int, gates, a, b, out, count, stream) }
                               else { tfhe_hip_pool_batch_gates_mixed_nks_dev(v, home as c_int, gates, a, b, out, count, stream) }, ()));
    }
    /// Drain what the device-resident calls enqueued on the members' own streams.
    pub fn synchronize(&self) { Self::check(self.pool, unsafe { tfhe_hip_pool_synchronize(self.pool) }); }
    /// "rccl" / "peer-copy" / "none": how the last device-resident call moved its shards.
    pub fn data_transport(&self) -> &'static str {
        unsafe { std::ffi::CStr::from_ptr(tfhe_hip_pool_data_transport(self.pool)) }.to_str().unwrap_or("?")
    }

    /// CloudKey::new(&secret_key) on the GPU (src/key.rs:59-66): replaces the sequential key-switching-key loop
    /// of key.rs:107-119 (the slowest user-visible step of the reference) and the 172 MB upload.  Masks and noise
    /// are a ChaCha20 stream under 32 bytes drawn from the crate's own CSPRNG -- `rand::rngs::OsRng`, the source
    /// thread_rng is seeded from -- never from a fixed seed: whoever can regenerate the noise reads the secret key
    /// off the published key rows.  The key is generated in a FRESH key view (no other call can see or disturb it)
    /// and read back in the reference layouts; the caller builds its CloudKey from the flat arrays (the inverse of
    /// `upload`) and the view is dropped -- or kept registered under the new CloudKey's address to skip the first upload.
    pub fn gen_cloud_key(&self, sk: &crate::key::SecretKey) -> (Vec<f64>, Vec<u32>, u32, Vec<u32>) {
        use rand::RngCore;
        let mut rng_key = [0u8; 32];
        rand::rngs::OsRng.fill_bytes(&mut rng_key);
        let mut view = std::ptr::null_mut();
        assert_eq!(unsafe { tfhe_hip_pool_key_create(self.pool, &mut view) }, 0, "tfhe_hip_pool_key_create failed");
        Self::check(view, unsafe { tfhe_hip_pool_gen_cloud_key_with_key(view, sk.key_lv0.as_ptr(), sk.key_lv1.as_ptr(),
                                                                        params::tlwe_lv0::ALPHA, params::tlwe_lv1::ALPHA,
                                                                        rng_key.as_ptr()) });
        rng_key.iter_mut().for_each(|b| *b = 0);
        let n = params::tlwe_lv0::N;
        let mut bsk = vec![0f64; n * 2 * params::trgsw_lv1::L * 2 * N];
        let mut ksk = vec![0u32; N * params::trgsw_lv1::IKS_T * (1 << params::trgsw_lv1::BASEBIT) * W];
        let (mut off, mut tv) = (0u32, vec![0u32; 2 * N]);
        Self::check(view, unsafe { tfhe_hip_pool_export_cloud_key(view, 0, bsk.as_mut_ptr(), ksk.as_mut_ptr(), &mut off, tv.as_mut_ptr()) });
        unsafe { tfhe_hip_pool_destroy(view) };
        (bsk, ksk, off, tv)
    }

    /// A seeded (compressed) cloud key, the format of include/tfhe_hip.h: the public 32-byte mask seed, the BSK bodies
    /// [n][2l][N] and the KSK bodies [N][t][base] -- what a client ships, a tenth of the full key's bytes on
    /// SECURITY_128_BIT.  As `gen_cloud_key` above: loaded into a TEMPORARY key view of the pool (the masks regenerated
    /// on the device, the key expanded there), read back in the reference layouts, and the view dropped on every path;
    /// the caller builds its CloudKey from the flat arrays (the inverse of `upload`) and uses it like any other.
    pub fn load_compressed_cloud_key(&self, mask_seed: &[u8; 32], bsk_bodies: &[u32], ksk_bodies: &[u32],
                                     decomp_offset: u32, testvec: &[u32]) -> (Vec<f64>, Vec<u32>, u32, Vec<u32>) {
        let n = params::tlwe_lv0::N;
        assert_eq!(bsk_bodies.len(), n * 2 * params::trgsw_lv1::L * N, "bsk_bodies is [n][2l][N]");
        assert_eq!(ksk_bodies.len(), N * params::trgsw_lv1::IKS_T * (1 << params::trgsw_lv1::BASEBIT), "ksk_bodies is [N][t][base]");
        assert_eq!(testvec.len(), 2 * N, "testvec is [2][N]");
        let mut bsk = vec![0f64; n * 2 * params::trgsw_lv1::L * 2 * N];
        let mut ksk = vec![0u32; N * params::trgsw_lv1::IKS_T * (1 << params::trgsw_lv1::BASEBIT) * W];
        let (mut off, mut tv) = (0u32, vec![0u32; 2 * N]);
        let mut view = std::ptr::null_mut();
        assert_eq!(unsafe { tfhe_hip_pool_key_create(self.pool, &mut view) }, 0, "tfhe_hip_pool_key_create failed");
        let mut rc = unsafe { tfhe_hip_pool_load_compressed_cloud_key(view, mask_seed.as_ptr(), bsk_bodies.as_ptr(),
                                                                      ksk_bodies.as_ptr(), decomp_offset, testvec.as_ptr()) };
        if rc == 0 {
            rc = unsafe { tfhe_hip_pool_export_cloud_key(view, 0, bsk.as_mut_ptr(), ksk.as_mut_ptr(), &mut off, tv.as_mut_ptr()) };
        }
        let msg = if rc == 0 { String::new() }
                  else { format!("{}", unsafe { std::ffi::CStr::from_ptr(tfhe_hip_pool_last_error(view)) }.to_string_lossy()) };
        unsafe { tfhe_hip_pool_destroy(view) };   // before any panic: the view never outlives the call
        assert_eq!(rc, 0, "tfhe_hip: {}", msg);
        (bsk, ksk, off, tv)
    }

    /// Packing key switch, the format of include/tfhe_hip.h: `cts` ([count][n+1] lv0 results, flat) become
    /// ceil(count / N) TRLWE lv1 [G][2][N] under the client's s1, each coefficient the phase of one input -- 350x fewer
    /// bytes to return on SECURITY_128_BIT.  The packing key (the public 32-byte mask seed and the bodies [n][t][N], made
    /// by the client) stays resident in a key view of the pool of its own and is loaded again only when another key
    /// (content sample) is passed, as the C++ mirror's `Engine::pack`; no cloud key is needed.
    pub fn pack_tlwe(&self, mask_seed: &[u8; 32], bodies: &[u32], cts: &[u32]) -> Vec<u32> {
        let n = params::tlwe_lv0::N;
        assert_eq!(bodies.len(), n * params::trgsw_lv1::IKS_T * N, "bodies is [n][t][N]");
        assert_eq!(cts.len() % W, 0, "cts is [count][n+1]");
        let count = cts.len() / W;
        let mut out = vec![0u32; (count + N - 1) / N * 2 * N];
        let mut g = self.packing.lock().unwrap();   // held through the pack: a concurrent call cannot swap the key
        self.packing_view(&mut g, mask_seed, bodies);
        Self::check(g.view, unsafe { tfhe_hip_pool_batch_pack_tlwe(g.view, cts.as_ptr(), count, out.as_mut_ptr()) });
        out
    }

    /// The packing key's own view holds (mask_seed, bodies): created on first use, loaded again only for another key.
    fn packing_view(&self, g: &mut PackingView, mask_seed: &[u8; 32], bodies: &[u32]) {
        let fp = Self::packing_fingerprint(mask_seed, bodies);
        if g.view.is_null() {
            let mut view = std::ptr::null_mut();
            assert_eq!(unsafe { tfhe_hip_pool_key_create(self.pool, &mut view) }, 0, "tfhe_hip_pool_key_create failed");
            g.view = view;
            g.fp = fp ^ 1;   // (nothing loaded yet)
        }
        if g.fp != fp {
            g.fp = fp ^ 1;   // a failed load leaves no key claimed
            Self::check(g.view, unsafe { tfhe_hip_pool_load_packing_key(g.view, mask_seed.as_ptr(), bodies.as_ptr()) });
            g.fp = fp;
        }
    }

    /// The packing key of the secret key (key_lv0 [n], key_lv1 [N]), generated on the GPU (`tfhe_hip_pool_gen_packing_key`,
    /// the format of include/tfhe_hip.h): returns (the public mask seed, the bodies [n][t][N]).  A client-side call, as the
    /// cloud-key generation is.  `alpha`: the noise's standard deviation (params::trgsw_lv1::ALPHA is the set's);
    /// `rng_key`: the 32-byte generator key from the caller's CSPRNG, None draws it from getrandom(2).  The packing key's
    /// view is left loaded with the key and its content sample set: `pack_tlwe` with the returned pair uploads nothing.
    pub fn gen_packing_key(&self, key_lv0: &[u32], key_lv1: &[u32], alpha: f64, rng_key: Option<&[u8; 32]>) -> ([u8; 32], Vec<u32>) {
        let n = params::tlwe_lv0::N;
        assert_eq!(key_lv0.len(), n, "key_lv0 is [n]");
        assert_eq!(key_lv1.len(), N, "key_lv1 is [N]");
        let mut seed = [0u8; 32];
        let mut bodies = vec![0u32; n * params::trgsw_lv1::IKS_T * N];
        let mut g = self.packing.lock().unwrap();   // held through the call: a concurrent pack cannot meet half a key
        if g.view.is_null() {
            let mut view = std::ptr::null_mut();
            assert_eq!(unsafe { tfhe_hip_pool_key_create(self.pool, &mut view) }, 0, "tfhe_hip_pool_key_create failed");
            g.view = view;
        }
        g.fp = !g.fp;   // a failed call leaves the key it replaces unclaimed (the next pack_tlwe loads again)
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check(g.view, unsafe {
            tfhe_hip_pool_gen_packing_key(g.view, key_lv0.as_ptr(), key_lv1.as_ptr(), alpha, rk, seed.as_mut_ptr(), bodies.as_mut_ptr())
        });
        g.fp = Self::packing_fingerprint(&seed, &bodies);
        (seed, bodies)
    }

    fn check_ctx(ctx: *mut TfheHipCtx, rc: c_int) {
        if rc != 0 {
            let msg = unsafe { std::ffi::CStr::from_ptr(tfhe_hip_last_error(ctx)) };
            panic!("tfhe_hip: {}", msg.to_string_lossy());
        }
    }

    /// The first member's context of the public key's view (created on first use).
    fn public_key_ctx(&self, g: &mut PackingView) -> *mut TfheHipCtx {
        if g.view.is_null() {
            let mut view = std::ptr::null_mut();
            assert_eq!(unsafe { tfhe_hip_pool_key_create(self.pool, &mut view) }, 0, "tfhe_hip_pool_key_create failed");
            g.view = view;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(g.view, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        ctx
    }

    /// PublicKeyLv0::encryptions, flat [size][n+1] with 1 <= size <= 8192, onto the public key's view
    /// (`tfhe_hip_load_public_key`): what `pk_encrypt` and `gen_reenc_key_asymmetric` below encrypt under.
    pub fn load_public_key(&self, encryptions: &[u32]) {
        assert!(!encryptions.is_empty() && encryptions.len() % W == 0, "encryptions is [size][n+1]");
        let mut g = self.public_key.lock().unwrap();   // held through the call: a concurrent encryption cannot meet half a key
        let ctx = self.public_key_ctx(&mut g);
        g.fp = 0;
        Self::check_ctx(ctx, unsafe { tfhe_hip_load_public_key(ctx, encryptions.as_ptr(), encryptions.len() / W) });
        g.fp = (encryptions.len() / W) as u64;
    }

    /// PublicKeyLv0::encrypt_f64 over a batch on the GPU, in the keyed format of include/tfhe_hip.h: `plain` are torus
    /// words (f64_to_torus of the messages), ciphertext m is row `first_index + m` of the generator key's streams.
    /// `rng_key`: the 32-byte generator key from the caller's CSPRNG, None draws it from getrandom(2).  A (rng_key, row)
    /// pair must never encrypt two messages.  Returns [count][n+1], flat.
    pub fn pk_encrypt(&self, plain: &[u32], alpha: f64, rng_key: Option<&[u8; 32]>, first_index: u64) -> Vec<u32> {
        let mut out = vec![0u32; plain.len() * W];
        let mut g = self.public_key.lock().unwrap();
        assert!(g.fp != 0, "no public key loaded: call load_public_key first");
        let ctx = self.public_key_ctx(&mut g);
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_pk_encrypt(ctx, plain.as_ptr(), plain.len(), alpha, rk, first_index, out.as_mut_ptr())
        });
        out
    }

    /// ProxyReencryptionKey::new_asymmetric (src/proxy_reenc.rs:271-326) from `key_from` (the delegator's key_lv0 [n])
    /// towards the loaded public key, generated on the GPU (`tfhe_hip_gen_reenc_key_asymmetric`): returns
    /// key_encryptions [n][t][base][n+1], flat, and leaves the public key's view holding the key, so that
    /// `reencrypt_generated` uploads nothing.  A client-side call: it takes a secret key.
    pub fn gen_reenc_key_asymmetric(&self, key_from: &[u32], alpha: f64, rng_key: Option<&[u8; 32]>) -> Vec<u32> {
        let n = params::tlwe_lv0::N;
        assert_eq!(key_from.len(), n, "key_from is [n]");
        let mut key = vec![0u32; n * params::trgsw_lv1::IKS_T * (1usize << params::trgsw_lv1::BASEBIT) * W];
        let mut g = self.public_key.lock().unwrap();
        assert!(g.fp != 0, "no public key loaded: call load_public_key first");
        let ctx = self.public_key_ctx(&mut g);
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, unsafe { tfhe_hip_gen_reenc_key_asymmetric(ctx, key_from.as_ptr(), alpha, rk, key.as_mut_ptr()) });
        key
    }

    /// TLWELv0::encrypt_f64 over a batch on the GPU, in the keyed format of include/tfhe_hip.h ("symmetric encryption",
    /// `tfhe_hip_batch_encrypt`): `plain` are torus words, ciphertext m is row `first_index + m`, its mask under the
    /// PUBLIC `mask_seed`, its noise under `rng_key` (the secret 32-byte generator key; None draws it from
    /// getrandom(2)).  Neither a (rng_key, row) nor a (mask_seed, row) pair may encrypt twice.  Returns [count][n+1],
    /// flat; with `bodies` the seeded form's bodies [count] are written there too.  Runs on the pool's first member.
    pub fn encrypt_batch(&self, key_lv0: &[u32], plain: &[u32], alpha: f64, rng_key: Option<&[u8; 32]>,
                         mask_seed: &[u8; 32], first_index: u64, bodies: Option<&mut [u32]>) -> Vec<u32> {
        assert_eq!(key_lv0.len(), params::tlwe_lv0::N, "key_lv0 is [n]");
        let mut out = vec![0u32; plain.len() * W];
        let bp = match bodies {
            Some(b) => { assert_eq!(b.len(), plain.len(), "bodies is [count]"); b.as_mut_ptr() }
            None => std::ptr::null_mut(),
        };
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_encrypt(ctx, key_lv0.as_ptr(), plain.as_ptr(), plain.len(), alpha, rk, mask_seed.as_ptr(),
                                   first_index, bp, out.as_mut_ptr())
        });
        out
    }

    /// Decryption of a batch on the GPU (include/tfhe_hip.h "decryption", `tfhe_hip_batch_decrypt`): `cts` is
    /// [count][key.len()+1], flat, under `key` -- key_lv0 [n] for TLWELv0 ciphertexts, key_lv1 [N] for lv1 rows of N + 1
    /// words.  Returns [count] words in every mode (DECRYPT_PHASE / DECRYPT_BOOL / DECRYPT_MESSAGE; `modulus` is read
    /// in message mode only): what TLWELv0::decrypt_bool / decrypt_lwe_message give one ciphertext at a time.  A
    /// client-side call: it takes a secret key.  Runs on the pool's first member.
    pub fn decrypt_batch(&self, key: &[u32], cts: &[u32], mode: c_int, modulus: u32) -> Vec<u32> {
        assert!(key.len() == params::tlwe_lv0::N || key.len() == N, "key is key_lv0 [n] or key_lv1 [N]");
        assert_eq!(cts.len() % (key.len() + 1), 0, "cts is [count][key.len()+1]");
        let count = cts.len() / (key.len() + 1);
        let mut out = vec![0u32; count];
        if count == 0 {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_decrypt(ctx, key.as_ptr(), key.len(), cts.as_ptr(), count, mode, modulus, out.as_mut_ptr())
        });
        out
    }
    /// The same on device pointers of the first member's GPU (`key` stays host memory), queued on `stream`: `cts` is
    /// [count][key.len()+1], `out` [count].  Safety: the pointers must stay valid until the work has run.
    pub unsafe fn decrypt_batch_dev(&self, key: &[u32], cts: *const u32, count: usize, mode: c_int, modulus: u32,
                                    out: *mut u32, stream: *mut c_void) {
        let ctx = tfhe_hip_pool_ctx(self.pool, 0);
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, tfhe_hip_batch_decrypt_dev(ctx, key.as_ptr(), key.len(), cts, count, mode, modulus, out, stream));
    }
    /// The first `count` slots of packed TRLWE lv1 ciphertexts ([groups][2][N], flat) under `key_lv1`
    /// (`tfhe_hip_batch_decrypt_trlwe`): result i is slot i % N of group i / N.  Returns [count] words as `decrypt_batch`.
    pub fn decrypt_trlwe(&self, key_lv1: &[u32], trlwe: &[u32], count: usize, mode: c_int, modulus: u32) -> Vec<u32> {
        assert_eq!(key_lv1.len(), N, "key_lv1 is [N]");
        assert_eq!(trlwe.len() % (2 * N), 0, "trlwe is [groups][2][N]");
        assert!(count <= trlwe.len() / 2, "count exceeds the slots of the packed ciphertexts");
        let mut out = vec![0u32; count];
        if count == 0 {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_decrypt_trlwe(ctx, key_lv1.as_ptr(), trlwe.as_ptr(), trlwe.len() / (2 * N), count, mode, modulus,
                                         out.as_mut_ptr())
        });
        out
    }
    /// The same on device pointers of the first member's GPU, queued on `stream`.  Safety: as `decrypt_batch_dev`.
    pub unsafe fn decrypt_trlwe_dev(&self, key_lv1: &[u32], trlwe: *const u32, groups: usize, count: usize, mode: c_int,
                                    modulus: u32, out: *mut u32, stream: *mut c_void) {
        assert_eq!(key_lv1.len(), N, "key_lv1 is [N]");
        let ctx = tfhe_hip_pool_ctx(self.pool, 0);
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, tfhe_hip_batch_decrypt_trlwe_dev(ctx, key_lv1.as_ptr(), trlwe, groups, count, mode, modulus, out, stream));
    }

    /// TRLWELv1::encrypt_f64 over a batch on the GPU, N values to a ciphertext, in the keyed format of include/tfhe_hip.h
    /// ("packed encryption", `tfhe_hip_batch_encrypt_trlwe`): `plain` are torus words, group m has index
    /// `first_group + m`, its mask under the PUBLIC `mask_seed`, its noise under `rng_key` (the secret 32-byte generator
    /// key; None draws it from getrandom(2)); the unused slots of the last group encrypt 0.  Neither a (rng_key, group)
    /// nor a (mask_seed, group) pair may encrypt twice.  Returns [groups][2][N], flat; with `bodies` the seeded form's
    /// bodies [groups][N] are written there too.  Runs on the pool's first member.
    pub fn encrypt_trlwe(&self, key_lv1: &[u32], plain: &[u32], alpha: f64, rng_key: Option<&[u8; 32]>,
                         mask_seed: &[u8; 32], first_group: u64, bodies: Option<&mut [u32]>) -> Vec<u32> {
        assert_eq!(key_lv1.len(), N, "key_lv1 is [N]");
        let groups = (plain.len() + N - 1) / N;
        let mut out = vec![0u32; groups * 2 * N];
        let bp = match bodies {
            Some(b) => { assert_eq!(b.len(), groups * N, "bodies is [groups][N]"); b.as_mut_ptr() }
            None => std::ptr::null_mut(),
        };
        if groups == 0 {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_encrypt_trlwe(ctx, key_lv1.as_ptr(), plain.as_ptr(), plain.len(), alpha, rk, mask_seed.as_ptr(),
                                         first_group, bp, out.as_mut_ptr())
        });
        out
    }
    /// The same on device pointers of the first member's GPU (`key_lv1` stays host memory), queued on `stream`: `plain`
    /// is [count], `bodies` [groups][N] and `out` [groups][2][N], either of the two may be null.  Safety: as
    /// `decrypt_batch_dev`.
    pub unsafe fn encrypt_trlwe_dev(&self, key_lv1: &[u32], plain: *const u32, count: usize, alpha: f64,
                                    rng_key: Option<&[u8; 32]>, mask_seed: &[u8; 32], first_group: u64, bodies: *mut u32,
                                    out: *mut u32, stream: *mut c_void) {
        assert_eq!(key_lv1.len(), N, "key_lv1 is [N]");
        let ctx = tfhe_hip_pool_ctx(self.pool, 0);
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, tfhe_hip_batch_encrypt_trlwe_dev(ctx, key_lv1.as_ptr(), plain, count, alpha, rk, mask_seed.as_ptr(),
                                                              first_group, bodies, out, stream));
    }
    /// A seeded packed batch (`mask_seed`, `first_group`, `bodies` [groups][N], flat) expanded on the GPU to the words
    /// the full form writes, [groups][2][N] (`tfhe_hip_expand_seeded_trlwe`).  No secret is involved.
    pub fn expand_seeded_trlwe(&self, mask_seed: &[u8; 32], first_group: u64, bodies: &[u32]) -> Vec<u32> {
        assert_eq!(bodies.len() % N, 0, "bodies is [groups][N]");
        let mut out = vec![0u32; bodies.len() * 2];
        if bodies.is_empty() {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_expand_seeded_trlwe(ctx, mask_seed.as_ptr(), first_group, bodies.as_ptr(), bodies.len() / N, out.as_mut_ptr())
        });
        out
    }
    /// The same on device pointers of the first member's GPU, queued on `stream`.  Safety: as `decrypt_batch_dev`.
    pub unsafe fn expand_seeded_trlwe_dev(&self, mask_seed: &[u8; 32], first_group: u64, bodies: *const u32, groups: usize,
                                          out: *mut u32, stream: *mut c_void) {
        let ctx = tfhe_hip_pool_ctx(self.pool, 0);
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, tfhe_hip_expand_seeded_trlwe_dev(ctx, mask_seed.as_ptr(), first_group, bodies, groups, out, stream));
    }

    /// A TRLWE switching key (include/tfhe_hip.h, "TRLWE key switch") from ring key `key_from` [N] to `key_to` [N] for the
    /// automorphism X -> X^k, generated on the GPU (`tfhe_hip_gen_trlwe_switch_key`): returns (the public mask seed, the
    /// bodies [t][N]) and leaves the key loaded under k on the pool's first member.  k = 1 with two different keys is the
    /// packed re-encryption key, k != 1 with the same key twice a Galois key.  A client-side call: it takes secret keys.
    /// `alpha`: the noise's standard deviation (params::trgsw_lv1::ALPHA is the set's); `rng_key`: the 32-byte generator
    /// key (one key per k under it), None draws it from getrandom(2).
    pub fn gen_trlwe_switch_key(&self, key_from: &[u32], key_to: &[u32], k: c_int, basebit: c_int, t: c_int, alpha: f64,
                                rng_key: Option<&[u8; 32]>) -> ([u8; 32], Vec<u32>) {
        assert_eq!(key_from.len(), N, "key_from is [N]");
        assert_eq!(key_to.len(), N, "key_to is [N]");
        let mut words: usize = 0;
        assert_eq!(unsafe { tfhe_hip_trlwe_switch_key_words(t, &mut words) }, 0, "t is out of range");
        let mut seed = [0u8; 32];
        let mut bodies = vec![0u32; words];
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let rk = rng_key.map_or(std::ptr::null(), |key| key.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_gen_trlwe_switch_key(ctx, key_from.as_ptr(), key_to.as_ptr(), k, basebit, t, alpha, rk, seed.as_mut_ptr(),
                                          bodies.as_mut_ptr())
        });
        (seed, bodies)
    }
    /// (mask_seed, bodies [t][N]) of a switching key expanded on the pool's first member and held there under k
    /// (`tfhe_hip_load_trlwe_switch_key`); up to 16 keys a handle, a key for the same k is replaced.
    pub fn load_trlwe_switch_key(&self, k: c_int, basebit: c_int, t: c_int, mask_seed: &[u8; 32], bodies: &[u32]) {
        let mut words: usize = 0;
        assert_eq!(unsafe { tfhe_hip_trlwe_switch_key_words(t, &mut words) }, 0, "t is out of range");
        assert_eq!(bodies.len(), words, "bodies is [t][N]");
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, unsafe { tfhe_hip_load_trlwe_switch_key(ctx, k, basebit, t, mask_seed.as_ptr(), bodies.as_ptr()) });
    }
    /// psi_k of packed ciphertexts ([count][2][N], flat) under the key loaded for k, under that key's target secret
    /// (`tfhe_hip_batch_trlwe_keyswitch`).  Returns [count][2][N], flat.  Runs on the pool's first member.
    pub fn trlwe_keyswitch(&self, k: c_int, trlwe: &[u32]) -> Vec<u32> {
        assert_eq!(trlwe.len() % (2 * N), 0, "trlwe is [count][2][N]");
        let mut out = vec![0u32; trlwe.len()];
        if trlwe.is_empty() {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        Self::check_ctx(ctx, unsafe { tfhe_hip_batch_trlwe_keyswitch(ctx, k, trlwe.as_ptr(), trlwe.len() / (2 * N), out.as_mut_ptr()) });
        out
    }

    /// trgsw::cmux (src/trgsw.rs:173-196) over packed ciphertexts under ONE caller-held TRGSW `sel` [2t][2][N] of gadget
    /// (basebit, t): d0 + sel (.) (d1 - d0) on [count][2][N] (flat), or with `d0` None the external product sel (.) d1
    /// (`tfhe_hip_batch_trlwe_cmux`).  `flags`: 0, or CMUX_REFERENCE_DIGITS.  Needs no key.  Runs on the pool's first
    /// member.
    pub fn trlwe_cmux(&self, sel: &[u32], basebit: c_int, t: c_int, flags: c_int, d0: Option<&[u32]>, d1: &[u32]) -> Vec<u32> {
        assert!(t >= 1 && sel.len() == 2 * (t as usize) * 2 * N, "sel is [2t][2][N]");
        assert_eq!(d1.len() % (2 * N), 0, "d1 is [count][2][N]");
        if let Some(a) = d0 {
            assert_eq!(a.len(), d1.len(), "d0 has d1's shape");
        }
        let mut out = vec![0u32; d1.len()];
        if d1.is_empty() {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let p0 = d0.map_or(std::ptr::null(), |a| a.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_trlwe_cmux(ctx, sel.as_ptr(), basebit, t, flags, p0, d1.as_ptr(), d1.len() / (2 * N), out.as_mut_ptr())
        });
        out
    }
    /// TRGSWLv1::encrypt_torus (src/trgsw.rs:29-49) for message polynomials: `mu` [count][N] small integers -> count
    /// selectors [count][2t][2][N] (flat) under `key_lv1` [N], made on the GPU (`tfhe_hip_batch_encrypt_trgsw`).  Row
    /// `row` of selector m takes index first_index + m 2t + row; a (rng_key, index) pair must never encrypt twice.
    /// `rng_key`: the 32-byte generator key, None draws it from getrandom(2).  A client-side call: it takes the secret key.
    pub fn encrypt_trgsw(&self, key_lv1: &[u32], mu: &[i32], basebit: c_int, t: c_int, alpha: f64, rng_key: Option<&[u8; 32]>,
                         first_index: u64) -> Vec<u32> {
        assert_eq!(key_lv1.len(), N, "key_lv1 is [N]");
        assert_eq!(mu.len() % N, 0, "mu is [count][N]");
        assert!(t >= 1 && t <= 32, "1 <= t <= 32");
        let count = mu.len() / N;
        let mut out = vec![0u32; count * 2 * (t as usize) * 2 * N];
        if count == 0 {
            return out;
        }
        let ctx = unsafe { tfhe_hip_pool_ctx(self.pool, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let rk = rng_key.map_or(std::ptr::null(), |key| key.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_batch_encrypt_trgsw(ctx, key_lv1.as_ptr(), mu.as_ptr(), count, basebit, t, alpha, rk, first_index,
                                         std::ptr::null_mut(), out.as_mut_ptr())
        });
        out
    }

    /// PublicKeyLv0::new_with_params (src/proxy_reenc.rs:144-153) on the GPU (`tfhe_hip_gen_public_key`): `size`
    /// encryptions of zero under `key_lv0`, returned flat [size][n+1] and left loaded on the public key's view, so that
    /// `pk_encrypt` and `gen_reenc_key_asymmetric` upload nothing.  One rng_key makes one public key.
    pub fn gen_public_key(&self, key_lv0: &[u32], size: usize, alpha: f64, rng_key: Option<&[u8; 32]>) -> Vec<u32> {
        assert_eq!(key_lv0.len(), params::tlwe_lv0::N, "key_lv0 is [n]");
        assert!(size >= 1 && size <= 8192, "1 <= size <= 8192");
        let mut enc = vec![0u32; size * W];
        let mut g = self.public_key.lock().unwrap();
        let ctx = self.public_key_ctx(&mut g);
        g.fp = 0;
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, unsafe { tfhe_hip_gen_public_key(ctx, key_lv0.as_ptr(), size, alpha, rk, enc.as_mut_ptr()) });
        g.fp = size as u64;
        enc
    }

    /// ProxyReencryptionKey::new_symmetric (src/proxy_reenc.rs:362-425) from `key_from` to `key_to` (both key_lv0 [n]),
    /// generated on the GPU (`tfhe_hip_gen_reenc_key_symmetric`): returns key_encryptions [n][t][base][n+1], flat, and
    /// leaves the public key's view holding the key, so that `reencrypt_generated` uploads nothing.
    pub fn gen_reenc_key_symmetric(&self, key_from: &[u32], key_to: &[u32], alpha: f64, rng_key: Option<&[u8; 32]>) -> Vec<u32> {
        let n = params::tlwe_lv0::N;
        assert!(key_from.len() == n && key_to.len() == n, "key_from and key_to are [n]");
        let mut key = vec![0u32; n * params::trgsw_lv1::IKS_T * (1usize << params::trgsw_lv1::BASEBIT) * W];
        let mut g = self.public_key.lock().unwrap();
        let ctx = self.public_key_ctx(&mut g);
        let rk = rng_key.map_or(std::ptr::null(), |k| k.as_ptr());
        Self::check_ctx(ctx, unsafe {
            tfhe_hip_gen_reenc_key_symmetric(ctx, key_from.as_ptr(), key_to.as_ptr(), alpha, rk, key.as_mut_ptr())
        });
        key
    }

    /// reencrypt_tlwe_lv0 over `cts` ([count][n+1], flat) under the key `gen_reenc_key_asymmetric` or
    /// `gen_reenc_key_symmetric` left on the view.
    pub fn reencrypt_generated(&self, cts: &[u32]) -> Vec<u32> {
        assert_eq!(cts.len() % W, 0, "cts is [count][n+1]");
        let mut out = vec![0u32; cts.len()];
        let mut g = self.public_key.lock().unwrap();
        let ctx = self.public_key_ctx(&mut g);
        Self::check_ctx(ctx, unsafe { tfhe_hip_batch_reencrypt(ctx, cts.as_ptr(), out.as_mut_ptr(), cts.len() / W) });
        out
    }

    /// Encrypted-table key switch, the definition of include/tfhe_hip.h: `stage1` ([m][count][n+1] lv0 ciphertexts, flat,
    /// function-major -- what the many-LUT bootstrap writes) becomes `count` encrypted test vectors [count][2][N] under
    /// s1, each the generator's table of its m inputs' phases.  Runs on the first member of the packing key's view (the
    /// call has no pool form); the packing key as in `pack_tlwe`.
    pub fn pack_table(&self, mask_seed: &[u8; 32], bodies: &[u32], stage1: &[u32], m: usize) -> Vec<u32> {
        let n = params::tlwe_lv0::N;
        assert_eq!(bodies.len(), n * params::trgsw_lv1::IKS_T * N, "bodies is [n][t][N]");
        assert!(m > 0 && stage1.len() % (m * W) == 0, "stage1 is [m][count][n+1]");
        let count = stage1.len() / (m * W);
        let mut out = vec![0u32; count * 2 * N];
        let mut g = self.packing.lock().unwrap();   // held through the call: a concurrent call cannot swap the key
        self.packing_view(&mut g, mask_seed, bodies);
        let ctx = unsafe { tfhe_hip_pool_ctx(g.view, 0) };
        assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
        let rc = unsafe { tfhe_hip_batch_pack_table(ctx, stage1.as_ptr(), m as c_int, count, out.as_mut_ptr()) };
        if rc != 0 {
            let msg = unsafe { std::ffi::CStr::from_ptr(tfhe_hip_last_error(ctx)) };
            panic!("tfhe_hip: {}", msg.to_string_lossy());
        }
        out
    }

    /// Tree bootstrap (tfhe_hip_pool_batch_bootstrap_bivariate): ciphertexts of f(x[c], y[c]) for digits of modulus `m`.
    /// `tables` is [m / n_luts][2][N], flat: table j packs f(j n_luts + r, .) for r < n_luts as the many-LUT generator
    /// does.  Runs under the key view of `ck`, where the packing key (mask_seed, bodies) is loaded beside the cloud key
    /// on first use and again only when another packing key (content sample) is passed.
    pub fn bootstrap_bivariate(&self, x: &[Ciphertext], y: &[Ciphertext], tables: &[u32], m: usize, n_luts: usize,
                               keyswitch: bool, mask_seed: &[u8; 32], bodies: &[u32], ck: &CloudKey) -> Vec<Ciphertext> {
        let n = params::tlwe_lv0::N;
        assert_eq!(bodies.len(), n * params::trgsw_lv1::IKS_T * N, "bodies is [n][t][N]");
        assert_eq!(x.len(), y.len(), "one y per x");
        assert!(n_luts > 0 && m % n_luts == 0 && tables.len() == m / n_luts * 2 * N, "tables is [m / n_luts][2][N]");
        let count = x.len();
        let (mut fx, mut fy, mut out) = (vec![0u32; count * W], vec![0u32; count * W], vec![0u32; count * W]);
        for (i, c) in x.iter().enumerate() { fx[i * W..(i + 1) * W].copy_from_slice(&c.p); }
        for (i, c) in y.iter().enumerate() { fy[i * W..(i + 1) * W].copy_from_slice(&c.p); }
        let pk_fp = Self::packing_fingerprint(mask_seed, bodies) | 1;   // (0 stands for "none loaded")
        self.with_key(ck, |v| {
            {   // under the registry lock, as a cloud-key upload: a second thread with the same keys waits here
                let mut g = self.views.lock().unwrap();
                if let Some(kv) = g.0.iter_mut().find(|kv| kv.view == v) {
                    if kv.pk_fp != pk_fp {
                        kv.pk_fp = 0;
                        let rc = unsafe { tfhe_hip_pool_load_packing_key(v, mask_seed.as_ptr(), bodies.as_ptr()) };
                        if rc != 0 { return (rc, ()); }
                        kv.pk_fp = pk_fp;
                    }
                }
            }
            (unsafe { tfhe_hip_pool_batch_bootstrap_bivariate(v, fx.as_ptr(), fy.as_ptr(), tables.as_ptr(), m as c_int,
                                                              n_luts as c_int, keyswitch as c_int, out.as_mut_ptr(), count) }, ())
        });
        Self::unflatten(&out)
    }

    /// Unpacking key switch, the definition of include/tfhe_hip.h: slots of `trlwe` ([groups][2][N] TRLWE lv1 under s1,
    /// flat -- what `pack_tlwe` returned, or what a client encrypted with `TRLWELv1::encrypt_bool`) become lv0 ciphertexts
    /// under `ck`'s key-switching key: `sample_extract_index(trlwe_G, j)` then `identity_key_switching` per slot.
    /// `slots = None` takes slots 0 .. count-1; otherwise output m takes slot `slots[m]` and `count` is ignored.
    pub fn unpack_trlwe(&self, trlwe: &[u32], slots: Option<&[u32]>, count: usize, ck: &CloudKey) -> Vec<Ciphertext> {
        assert_eq!(trlwe.len() % (2 * N), 0, "trlwe is [groups][2][N]");
        let groups = trlwe.len() / (2 * N);
        let count = slots.map_or(count, |s| s.len());
        let sp = slots.map_or(std::ptr::null(), |s| s.as_ptr());
        let mut out = vec![0u32; count * W];
        self.with_key(ck, |v| (unsafe { tfhe_hip_pool_batch_unpack_trlwe(v, trlwe.as_ptr(), groups, sp, count, out.as_mut_ptr()) }, ()));
        Self::unflatten(&out)
    }
    /// The same on device pointers of member `home`'s GPU (`slots` too, or null); the call only enqueues and leaves the
    /// range of the slots to the caller.  Safety: the pointers must stay valid until the work has run (`synchronize`).
    pub unsafe fn unpack_trlwe_dev(&self, home: usize, trlwe: *const u32, groups: usize, slots: *const u32, count: usize,
                                   out: *mut u32, stream: *mut c_void, ck: &CloudKey) {
        self.with_key(ck, |v| (tfhe_hip_pool_batch_unpack_trlwe_dev(v, home as c_int, trlwe, groups, slots, count, out, stream), ()));
    }

    /// Encrypted linear layer, dense form (`tfhe_hip_batch_tlwe_matmul`): `w` is [rows][cols] int8 row-major, `input`
    /// [groups][cols][n+1] flat, `bias` [rows] torus words; returns [groups][rows][n+1] flat with
    /// out[g][r] = sum_j w[r][j] * input[g][j] + bias[r] on the body, exact mod 2^32.  Runs on the first member of `ck`'s
    /// key view (the call has no pool form; the product itself uses no key).
    pub fn tlwe_matmul(&self, w: &[i8], bias: Option<&[u32]>, rows: usize, cols: usize, input: &[u32], ck: &CloudKey) -> Vec<u32> {
        assert!(rows > 0 && cols > 0 && w.len() == rows * cols, "w is [rows][cols]");
        assert!(input.len() % (cols * W) == 0, "input is [groups][cols][n+1]");
        assert!(bias.map_or(true, |b| b.len() == rows), "bias is [rows]");
        let groups = input.len() / (cols * W);
        let bp = bias.map_or(std::ptr::null(), |b| b.as_ptr());
        let mut out = vec![0u32; groups * rows * W];
        self.with_key(ck, |v| {
            let ctx = unsafe { tfhe_hip_pool_ctx(v, 0) };
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, unsafe {
                tfhe_hip_batch_tlwe_matmul(ctx, w.as_ptr(), bp, rows, cols, input.as_ptr(), groups, out.as_mut_ptr())
            });
            (0, ())
        });
        out
    }
    /// The packed form (`tfhe_hip_batch_trlwe_matmul`): the same product on slots 0 .. cols-1 of every group of `trlwe`
    /// ([groups][2][N] flat), extracted with the exact wrapping negation.  `keyswitch`: [groups][rows][n+1] lv0
    /// ciphertexts under `ck`'s key-switching key; without, the lv1 rows [groups][rows][N+1].
    pub fn trlwe_matmul(&self, w: &[i8], bias: Option<&[u32]>, rows: usize, cols: usize, trlwe: &[u32], keyswitch: bool,
                        ck: &CloudKey) -> Vec<u32> {
        assert!(rows > 0 && cols > 0 && cols <= N && w.len() == rows * cols, "w is [rows][cols], cols <= N");
        assert_eq!(trlwe.len() % (2 * N), 0, "trlwe is [groups][2][N]");
        assert!(bias.map_or(true, |b| b.len() == rows), "bias is [rows]");
        let groups = trlwe.len() / (2 * N);
        let bp = bias.map_or(std::ptr::null(), |b| b.as_ptr());
        let mut out = vec![0u32; groups * rows * if keyswitch { W } else { N + 1 }];
        self.with_key(ck, |v| {
            let ctx = unsafe { tfhe_hip_pool_ctx(v, 0) };
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, unsafe {
                tfhe_hip_batch_trlwe_matmul(ctx, w.as_ptr(), bp, rows, cols, trlwe.as_ptr(), groups, keyswitch as c_int,
                                            out.as_mut_ptr())
            });
            (0, ())
        });
        out
    }
    /// Plaintext polynomial product on packed ciphertexts (`tfhe_hip_batch_trlwe_polymul`): `w` is [rows][cols][N] int8
    /// polynomials, `trlwe` [groups][cols][2][N] flat, `bias` [rows][N] torus words; returns [groups][rows][2][N] flat,
    /// out[g][r](X) = sum_j w[r][j](X) * trlwe[g][j](X) mod X^N + 1 on both components, + bias[r](X) on b, exact mod
    /// 2^32.  cols <= 64.  Runs on the first member of `ck`'s key view (no pool form; the product itself uses no key).
    pub fn trlwe_polymul(&self, w: &[i8], bias: Option<&[u32]>, rows: usize, cols: usize, trlwe: &[u32], ck: &CloudKey) -> Vec<u32> {
        assert!(rows > 0 && cols > 0 && cols <= 64 && w.len() == rows * cols * N, "w is [rows][cols][N], cols <= 64");
        assert_eq!(trlwe.len() % (cols * 2 * N), 0, "trlwe is [groups][cols][2][N]");
        assert!(bias.map_or(true, |b| b.len() == rows * N), "bias is [rows][N]");
        let groups = trlwe.len() / (cols * 2 * N);
        let bp = bias.map_or(std::ptr::null(), |b| b.as_ptr());
        let mut out = vec![0u32; groups * rows * 2 * N];
        self.with_key(ck, |v| {
            let ctx = unsafe { tfhe_hip_pool_ctx(v, 0) };
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, unsafe {
                tfhe_hip_batch_trlwe_polymul(ctx, w.as_ptr(), bp, rows, cols, trlwe.as_ptr(), groups, out.as_mut_ptr())
            });
            (0, ())
        });
        out
    }
    /// The same on device pointers of the first member's GPU (`w` and `bias` too; `bias` may be null), queued on
    /// `stream`.  Safety: the pointers must stay valid until the work has run.
    pub unsafe fn trlwe_polymul_dev(&self, w: *const i8, bias: *const u32, rows: usize, cols: usize, trlwe: *const u32,
                                    groups: usize, out: *mut u32, stream: *mut c_void, ck: &CloudKey) {
        self.with_key(ck, |v| {
            let ctx = tfhe_hip_pool_ctx(v, 0);
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, tfhe_hip_batch_trlwe_polymul_dev(ctx, w, bias, rows, cols, trlwe, groups, out, stream));
            (0, ())
        });
    }
    /// Encrypted 2-D convolution (`tfhe_hip_batch_tlwe_conv2d`): `w` is [out_c][k_h][k_w][in_c] int8, `input`
    /// [groups][in_h][in_w][in_c][n+1] flat (channels-last), `bias` [out_c] torus words; returns
    /// [groups][out_h][out_w][out_c][n+1] flat, every output the exact sum of its taps mod 2^32 with zeros outside the
    /// map.  Runs on the first member of `ck`'s key view (no pool form; the convolution itself uses no key).
    pub fn tlwe_conv2d(&self, shape: &TfheHipConv2dShape, w: &[i8], bias: Option<&[u32]>, input: &[u32], ck: &CloudKey) -> Vec<u32> {
        let (out_h, out_w) = shape.out_hw();
        let (in_c, out_c) = (shape.in_c as usize, shape.out_c as usize);
        let per_group = shape.in_h as usize * shape.in_w as usize * in_c * W;
        assert!(in_c > 0 && out_c > 0 && w.len() == out_c * shape.k_h as usize * shape.k_w as usize * in_c, "w is [out_c][k_h][k_w][in_c]");
        assert!(input.len() % per_group == 0, "input is [groups][in_h][in_w][in_c][n+1]");
        assert!(bias.map_or(true, |b| b.len() == out_c), "bias is [out_c]");
        let groups = input.len() / per_group;
        let bp = bias.map_or(std::ptr::null(), |b| b.as_ptr());
        let mut out = vec![0u32; groups * out_h * out_w * out_c * W];
        self.with_key(ck, |v| {
            let ctx = unsafe { tfhe_hip_pool_ctx(v, 0) };
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, unsafe {
                tfhe_hip_batch_tlwe_conv2d(ctx, shape, w.as_ptr(), bp, input.as_ptr(), groups, out.as_mut_ptr())
            });
            (0, ())
        });
        out
    }
    /// The same on device pointers of the first member's GPU (`w` and `bias` too; `bias` may be null), queued on
    /// `stream`.  Safety: the pointers must stay valid until the work has run.
    pub unsafe fn tlwe_conv2d_dev(&self, shape: &TfheHipConv2dShape, w: *const i8, bias: *const u32, input: *const u32,
                                  groups: usize, out: *mut u32, stream: *mut c_void, ck: &CloudKey) {
        self.with_key(ck, |v| {
            let ctx = tfhe_hip_pool_ctx(v, 0);
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, tfhe_hip_batch_tlwe_conv2d_dev(ctx, shape, w, bias, input, groups, out, stream));
            (0, ())
        });
    }
    /// Both forms on device pointers of the first member's GPU (`w` and `bias` too; `bias` may be null), queued on
    /// `stream`; `trlwe_input` selects the packed form.  Safety: the pointers must stay valid until the work has run.
    pub unsafe fn matmul_dev(&self, trlwe_input: bool, w: *const i8, bias: *const u32, rows: usize, cols: usize,
                             input: *const u32, groups: usize, keyswitch: bool, out: *mut u32, stream: *mut c_void,
                             ck: &CloudKey) {
        self.with_key(ck, |v| {
            let ctx = tfhe_hip_pool_ctx(v, 0);
            assert!(!ctx.is_null(), "tfhe_hip_pool_ctx failed");
            Self::check_ctx(ctx, if trlwe_input {
                tfhe_hip_batch_trlwe_matmul_dev(ctx, w, bias, rows, cols, input, groups, keyswitch as c_int, out, stream)
            } else {
                tfhe_hip_batch_tlwe_matmul_dev(ctx, w, bias, rows, cols, input, groups, out, stream)
            });
            (0, ())
        });
    }

    /// the seed, 64 evenly spaced body words and the size (FNV-style mix), as the C++ mirror samples a packing key
    fn packing_fingerprint(mask_seed: &[u8; 32], bodies: &[u32]) -> u64 {
        let mut h: u64 = 0x1656_67B1_9E37_79F9;
        let mut mix = |v: u64| { h = (h ^ v).wrapping_mul(0x0000_0100_0000_01B3); };
        for i in 0..32 { mix(mask_seed[i] as u64); }
        let nb = bodies.len();
        for i in 0..64 { mix(bodies[(nb - 1) * i / 64] as u64); }
        mix(nb as u64);
        h
    }
}
/// The process-wide engine behind `default_bootstrap()` and the `gates::batch_*` functions when the crate is built with
/// `--features hip`: created on first use over every GPU of the node -- the stand-in for `default_railgun()`'s "one
/// worker per logical CPU" (src/parallel/mod.rs:79-97, rayon_impl.rs:15-27) -- or over the devices listed in
/// `TFHE_HIP_DEVICES` ("0", "0,1,2,3", ...).  It lives for the rest of the process (as Rayon's global pool does).
pub fn default_engine() -> std::sync::Arc<HipEngine> {
    static ENGINE: std::sync::OnceLock<std::sync::Arc<HipEngine>> = std::sync::OnceLock::new();
    ENGINE.get_or_init(|| {
        let devices: Vec<i32> = match std::env::var("TFHE_HIP_DEVICES") {
            Ok(list) => list.split(',').map(|d| d.trim().parse().expect("TFHE_HIP_DEVICES: comma-separated device indices")).collect(),
            Err(_) => (0..unsafe { tfhe_hip_device_count() }).collect(),
        };
        assert!(!devices.is_empty(), "tfhe_hip: no GPU visible to this process");
        std::sync::Arc::new(HipEngine::new(&devices))
    }).clone()
}

impl Drop for HipEngine {
    fn drop(&mut self) {
        for v in self.views.lock().unwrap().0.drain(..) { unsafe { tfhe_hip_pool_destroy(v.view) } }   // views before their pool
        let pv = self.packing.lock().unwrap().view;
        if !pv.is_null() { unsafe { tfhe_hip_pool_destroy(pv) } }
        let kv = self.public_key.lock().unwrap().view;
        if !kv.is_null() { unsafe { tfhe_hip_pool_destroy(kv) } }
        unsafe { tfhe_hip_pool_destroy(self.pool) }
    }
}

/// The GPU stand-in for VanillaBootstrap (src/bootstrap/vanilla.rs:22-69); single calls are count = 1 batches
/// (they take the eight-waves-per-ciphertext latency kernel: 2.2 ms per gate).
pub struct HipBootstrap { engine: std::sync::Arc<HipEngine> }
impl HipBootstrap {
    /// `HipBootstrap::new()` mirrors `VanillaBootstrap::new()` (vanilla.rs:27-37): the process-wide engine.
    pub fn new() -> Self { HipBootstrap { engine: default_engine() } }
    pub fn with_engine(engine: std::sync::Arc<HipEngine>) -> Self { HipBootstrap { engine } }
    pub fn engine(&self) -> &std::sync::Arc<HipEngine> { &self.engine }
}
impl Default for HipBootstrap { fn default() -> Self { Self::new() } }

impl Bootstrap for HipBootstrap {
    fn bootstrap(&self, ctxt: &Ciphertext, cloud_key: &CloudKey) -> Ciphertext {
        self.engine.batch_bootstrap(std::slice::from_ref(ctxt), None, true, cloud_key).pop().unwrap()
    }
    fn bootstrap_without_key_switch(&self, ctxt: &Ciphertext, cloud_key: &CloudKey) -> Ciphertext {
        self.engine.batch_bootstrap(std::slice::from_ref(ctxt), None, false, cloud_key).pop().unwrap()
    }
    fn name(&self) -> &str { "hip-gfx950" }
}

/// src/bootstrap/lut.rs:24-126 on the GPU: the LUT's polynomial is the test vector of the blind rotation.
/// (Everything from here on needs the crate's `lut-bootstrap` feature, as `bootstrap::lut` itself does.)
#[cfg(feature = "lut-bootstrap")]
pub struct HipLutBootstrap { engine: std::sync::Arc<HipEngine> }
#[cfg(feature = "lut-bootstrap")]
impl HipLutBootstrap {
    /// mirrors `LutBootstrap::new()` (lut.rs:29-35): the process-wide engine
    pub fn new() -> Self { HipLutBootstrap { engine: default_engine() } }
    pub fn with_engine(engine: std::sync::Arc<HipEngine>) -> Self { HipLutBootstrap { engine } }
    /// lut.rs:49-65
    pub fn bootstrap_func<F: Fn(usize) -> usize>(&self, ct_in: &Ciphertext, f: F, message_modulus: usize, cloud_key: &CloudKey) -> Ciphertext {
        let lut = crate::lut::Generator::new(message_modulus).generate_lookup_table(f);
        self.bootstrap_lut(ct_in, &lut, cloud_key)
    }
    /// lut.rs:79-99
    pub fn bootstrap_lut(&self, ct_in: &Ciphertext, lut: &LookupTable, cloud_key: &CloudKey) -> Ciphertext {
        self.engine.batch_bootstrap(std::slice::from_ref(ct_in), Some(&lut.poly), true, cloud_key).pop().unwrap()
    }
    /// the batched form the GPU is meant to be fed with: one LUT, many ciphertexts
    pub fn batch_bootstrap_lut(&self, cts: &[Ciphertext], lut: &LookupTable, cloud_key: &CloudKey) -> Vec<Ciphertext> {
        self.engine.batch_bootstrap(cts, Some(&lut.poly), true, cloud_key)
    }
}
#[cfg(feature = "lut-bootstrap")]
impl Default for HipLutBootstrap { fn default() -> Self { Self::new() } }
#[cfg(feature = "lut-bootstrap")]
impl Bootstrap for HipLutBootstrap {
    fn bootstrap(&self, ctxt: &Ciphertext, cloud_key: &CloudKey) -> Ciphertext {     // lut.rs:108-111: identity, m = 2
        self.bootstrap_func(ctxt, |x| x, 2, cloud_key)
    }
    fn bootstrap_without_key_switch(&self, ctxt: &Ciphertext, cloud_key: &CloudKey) -> Ciphertext {   // lut.rs:113-121
        self.bootstrap(ctxt, cloud_key)
    }
    fn name(&self) -> &str { "lut-hip-gfx950" }
}

// ---- circuits: a gate / mux / LUT DAG scheduled by the library (include/tfhe_hip.h, tfhe_hip_circuit_*) ----------
#[repr(C)]
pub struct TfheHipCircuit { _private: [u8; 0] }

extern "C" {   // include/tfhe_hip.h, the tfhe_hip_circuit_* family: built on the host, levelised, run one launch per kind and level
    fn tfhe_hip_circuit_create(n_inputs: u32, out: *mut *mut TfheHipCircuit) -> c_int;
    fn tfhe_hip_circuit_destroy(circ: *mut TfheHipCircuit);
    fn tfhe_hip_circuit_add_gate(circ: *mut TfheHipCircuit, gate: c_int, a: u32, b: u32, wire: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_mux(circ: *mut TfheHipCircuit, a: u32, b: u32, c: u32, wire: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_lut(circ: *mut TfheHipCircuit, testvec: *const u32, lut: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_pbs(circ: *mut TfheHipCircuit, ca: u32, a: u32, cb: u32, b: u32, cconst: u32, lut: u32,
                                wire: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_pbs_many(circ: *mut TfheHipCircuit, ca: u32, a: u32, cb: u32, b: u32, cconst: u32, lut: u32,
                                     n_luts: c_int, wires: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_lincomb(circ: *mut TfheHipCircuit, coefs: *const u32, wires: *const u32, n_terms: usize,
                                    cconst: u32, wire: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_not(circ: *mut TfheHipCircuit, a: u32, wire: *mut u32) -> c_int;
    fn tfhe_hip_circuit_add_constant(circ: *mut TfheHipCircuit, value: c_int, wire: *mut u32) -> c_int;
    fn tfhe_hip_circuit_compile(circ: *mut TfheHipCircuit) -> c_int;
    fn tfhe_hip_circuit_run_pool(pool: *mut TfheHipPool, circ: *mut TfheHipCircuit, inputs: *const u32, batch: usize,
                                 out_wires: *const u32, n_out: usize, out: *mut u32) -> c_int;
}

/// A circuit over wires (0 .. n_inputs are its inputs; every node added returns its output wire), run by the library:
/// the reference evaluates examples/add_two_numbers.rs:11-50 one gate at a time, here every level of the DAG -- all of
/// its gates times the whole batch -- is one launch per kind, with the wires kept on the GPU between levels.
pub struct HipCircuit { h: *mut TfheHipCircuit, n_inputs: usize }
unsafe impl Send for HipCircuit {}   // the library serialises construction, compilation, and runs of one circuit on one pool (key views included)
unsafe impl Sync for HipCircuit {}

impl HipCircuit {
    pub fn new(n_inputs: usize) -> Self {
        let mut h = std::ptr::null_mut();
        assert_eq!(unsafe { tfhe_hip_circuit_create(n_inputs as u32, &mut h) }, 0, "tfhe_hip_circuit_create failed");
        HipCircuit { h, n_inputs }
    }
    fn node(rc: c_int, wire: u32) -> u32 {
        assert_eq!(rc, 0, "tfhe_hip_circuit: bad wire, gate code or lut id, or the circuit has already run");
        wire
    }
    /// Gates::<gate> (src/gates.rs:54-150), one of NAND .. COPY
    pub fn gate(&mut self, gate: c_int, a: u32, b: u32) -> u32 {
        let mut w = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_gate(self.h, gate, a, b, &mut w) };
        Self::node(rc, w)
    }
    /// Gates::mux (src/gates.rs:157-183)
    pub fn mux(&mut self, a: u32, b: u32, c: u32) -> u32 {
        let mut w = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_mux(self.h, a, b, c, &mut w) };
        Self::node(rc, w)
    }
    /// a test vector for `pbs` (LookupTable::poly, src/lut/lookup_table.rs); returns its id
    pub fn lut(&mut self, testvec: &trlwe::TRLWELv1) -> u32 {
        let mut tv = Vec::with_capacity(2 * N);
        tv.extend_from_slice(&testvec.a);
        tv.extend_from_slice(&testvec.b);
        let mut id = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_lut(self.h, tv.as_ptr(), &mut id) };
        Self::node(rc, id)
    }
    /// LutBootstrap::bootstrap_lut (src/bootstrap/lut.rs:79-99) of ca*a + cb*b + cconst
    pub fn pbs(&mut self, ca: u32, a: u32, cb: u32, b: u32, cconst: u32, lut: u32) -> u32 {
        let mut w = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_pbs(self.h, ca, a, cb, b, cconst, lut, &mut w) };
        Self::node(rc, w)
    }
    /// Many-LUT bootstrap: the n_luts (1, 2, 4 or 8) functions packed in `lut` of ca*a + cb*b + cconst from ONE blind
    /// rotation; returns the n_luts consecutive wires, function j at [j]
    pub fn pbs_many(&mut self, ca: u32, a: u32, cb: u32, b: u32, cconst: u32, lut: u32, n_luts: usize) -> Vec<u32> {
        let mut w = vec![0u32; n_luts];
        let rc = unsafe { tfhe_hip_circuit_add_pbs_many(self.h, ca, a, cb, b, cconst, lut, n_luts as c_int, w.as_mut_ptr()) };
        Self::node(rc, 0);
        w
    }
    /// sum coef * wire + cconst (TLWE `+` / `-`): no bootstrap
    pub fn lincomb(&mut self, terms: &[(u32, u32)], cconst: u32) -> u32 {
        let coefs: Vec<u32> = terms.iter().map(|t| t.0).collect();
        let wires: Vec<u32> = terms.iter().map(|t| t.1).collect();
        let mut w = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_lincomb(self.h, coefs.as_ptr(), wires.as_ptr(), terms.len(), cconst, &mut w) };
        Self::node(rc, w)
    }
    /// Gates::not (src/gates.rs:202-204)
    pub fn not(&mut self, a: u32) -> u32 {
        let mut w = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_not(self.h, a, &mut w) };
        Self::node(rc, w)
    }
    /// Gates::constant (src/gates.rs:212-219)
    pub fn constant(&mut self, value: bool) -> u32 {
        let mut w = 0u32;
        let rc = unsafe { tfhe_hip_circuit_add_constant(self.h, value as c_int, &mut w) };
        Self::node(rc, w)
    }
    /// examples/add_two_numbers.rs:11-29 -> (sum, carry)
    pub fn full_adder(&mut self, a: u32, b: u32, c: u32) -> (u32, u32) {
        let a_xor_b = self.gate(XOR, a, b);
        let a_and_b = self.gate(AND, a, b);
        let a_xor_b_and_c = self.gate(AND, a_xor_b, c);
        let sum = self.gate(XOR, a_xor_b, c);
        let carry = self.gate(OR, a_and_b, a_xor_b_and_c);
        (sum, carry)
    }
    /// examples/add_two_numbers.rs:31-50 -> (sum bits, carry out)
    pub fn add(&mut self, a: &[u32], b: &[u32], cin: u32) -> (Vec<u32>, u32) {
        assert_eq!(a.len(), b.len(), "Cannot add two numbers with different number of bits!");
        let mut result = Vec::with_capacity(a.len());
        let mut carry = cin;
        for (x, y) in a.iter().zip(b.iter()) {
            let (s, c) = self.full_adder(*x, *y, carry);
            result.push(s);
            carry = c;
        }
        (result, carry)
    }
    /// inputs[i][j]: input wire i of batch element j -> result[k][j]: wire out_wires[k] of batch element j, on `engine`'s
    /// GPUs under `cloud_key` (tfhe_hip_circuit_run_pool)
    pub fn run(&self, engine: &HipEngine, inputs: &[Vec<Ciphertext>], out_wires: &[u32], cloud_key: &CloudKey) -> Vec<Vec<Ciphertext>> {
        assert_eq!(inputs.len(), self.n_inputs, "one batch per circuit input");
        let batch = inputs[0].len();
        let mut flat = Vec::with_capacity(inputs.len() * batch * W);
        for row in inputs {
            assert_eq!(row.len(), batch, "inputs differ in batch size");
            for c in row { flat.extend_from_slice(&c.p); }
        }
        let mut out = vec![0u32; out_wires.len() * batch * W];
        let (h, outp) = (self.h, out.as_mut_ptr());
        engine.with_key(cloud_key, |v| (unsafe { tfhe_hip_circuit_run_pool(v, h, flat.as_ptr(), batch, out_wires.as_ptr(), out_wires.len(), outp) }, ()));
        out.chunks_exact(batch * W).map(HipEngine::unflatten).collect()
    }
}

impl Drop for HipCircuit {
    fn drop(&mut self) { unsafe { tfhe_hip_circuit_destroy(self.h) } }
}
