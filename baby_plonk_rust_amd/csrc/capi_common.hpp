// capi_common.hpp -- helpers shared by the capi_*.hip translation units (not part of the C ABI, not installed).
#pragma once
#include <functional>
#include <vector>

#include "commit_plan.hpp"      // shard_range, shard_cut, shard_slice: which points and scalars lie on which shard
#include "ctx.hpp"
#include "host_codec.hpp"

inline bool fmt_ok(int fmt) { return fmt == BP_FR_BYTES_LE || fmt == BP_FR_MONT; }
inline bool basis_ok(int b) { return b == BP_BASIS_LAGRANGE || b == BP_BASIS_MONOMIAL; }
// why a G1 point was rejected: `reason` of a decoder's status word (g1_check.hpp), for a 48-byte compressed record or a 96-byte one
inline const char* g1_reject_text(uint32_t reason, bool compressed) {
  if (reason == bp::G1_BAD_ENCODING) return compressed ? "bad encoding (flag bits, or x >= p)" : "bad encoding (flag bits, or a coordinate >= p)";
  if (reason == bp::G1_NOT_ON_CURVE) return compressed ? "not on the curve (x^3 + 4 has no square root)" : "not on the curve";
  return "not in the prime-order subgroup";
}
// one 96-byte record checked on the host: canonical, flags, on the curve (the checks of bp_srs_load); false = refused.  The identity
// (only a record with the infinity flag) passes as (0, 0).
inline bool host_point96(bp::g1_affine& out, const uint8_t in96[96]) {
  bp::g1_proj p;
  if (!bp::host_decode96(p, in96)) return false;
  if (bp::g1_is_identity(p)) {
    out.x = out.y = bp::Fp::zero();
    return true;
  }
  out.x = p.x;
  out.y = p.y;
  return bp::g1_affine_on_curve(out);
}
// (A, B) = (identity, identity): what a reduce of nothing returns
inline void encode_identity_pair(uint8_t out192[192]) {
  memset(out192, 0, 192);
  out192[0] = out192[96] = 0x40;
}
// capi_ctx.hip
// d_bad (bp::fr_bad_word): upload_fr raises it for a canonical-bytes input >= q; download_fr reads it with the copy that ends the
// call and returns BP_ERR_BAD_SCALAR when it is set (`host` is then unspecified)
int upload_fr(bp_ctx* ctx, const char* name, const void* host, size_t n, size_t cap_elems, int fmt, bp::fr_t** out, uint32_t* d_bad = nullptr);
int download_fr(bp_ctx* ctx, bp::fr_t* d, void* host, size_t n, int fmt, const uint32_t* d_bad = nullptr);
// work(r) for every member r for which use(r) holds: member 0 on the calling thread, the others on their own threads, all at once
void over_members(bp_ctx* ctx, size_t R, const std::function<bool(size_t)>& use, const std::function<void(size_t)>& work);
std::vector<bp_ctx*> shards_of(bp_ctx* ctx);
int ctx_create(bp_ctx** out, int device_id);
// capi_srs.hip
int srs_find(bp_ctx* ctx, uint64_t handle, bp::SrsEntry** out);
// A new entry of ctx (one device) over the resident points d: the 28-bit copy is made, the stream waited for.  Takes ownership of d
// (freed on failure); the entry covers global points [first, first + n) of an SRS of n_global points, Monomial until the caller says otherwise.
int srs_register(bp_ctx* ctx, bp::g1_affine* d, size_t n, size_t first, size_t n_global, uint64_t* handle);
int srs_free_one(bp_ctx* ctx, uint64_t handle);            // one member's entry and everything it holds
// One shard of an SRS: the member that holds it, the member's entry and handle, and the part [lo, hi) of the range asked for
// that lies on it, in global point indices (lo >= hi: none of it does).
struct SrsShard {
  bp_ctx* m;
  bp::SrsEntry* e;
  uint64_t handle;
  size_t lo, hi;
};
// The shards of the SRS `srs_handle` names on ctx (the leader of a group, or a plain context: one shard), in ascending point
// order, each with its part of points [first, first + n) cut to the SRS's length (default: every point).  A member's lookup error
// is lifted to ctx.  srs_shards_checked refuses a range that does not lie inside the SRS instead of cutting it.
int srs_shards(bp_ctx* ctx, uint64_t srs_handle, std::vector<SrsShard>* out, size_t first = 0, size_t n = SIZE_MAX);
int srs_shards_checked(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, std::vector<SrsShard>* out);
// capi_kzg_open_all.hip
// the SRS and shape rules of bp_kzg_open_cosets; on BP_OK *e is the SRS's entry (the leader's, for a group)
int open_cosets_srs_check(bp_ctx* ctx, uint64_t srs, uint32_t log_n, uint32_t log_l, bp::SrsEntry** e);
// The cells and cell proofs of n_values <= n Montgomery coefficients resident on the context's device, behind open_cosets_srs_check:
// what bp_kzg_open_cosets_device computes, with the results left in workspaces of the context.  *d_values_out (want_values): the n
// values in cell order; *d_bytes_out: the n / l x 96 proof bytes, or nullptr where the one proof is the identity (log_l == log_n).
// The stream has been waited for when *d_bytes_out is set, else the work is enqueued.
int open_cosets_resident(bp_ctx* ctx, uint64_t srs, bp::SrsEntry* e, const bp::fr_t* d_poly, size_t n_values, uint32_t log_n, uint32_t log_l,
                         bool want_values, bp::fr_t** d_values_out, uint8_t** d_bytes_out);
// does an MSM of n points against this entry go through its fixed-base tables?
bool srs_tables_pay(const bp::SrsEntry& e, size_t n);
