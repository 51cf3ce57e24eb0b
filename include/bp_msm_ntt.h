/*
 * bp_msm_ntt.h -- C ABI of the MI355X-native PLONK hot path (BLS12-381 G1 MSM + Fr NTT + polynomial ops).
 *
 * This is the drop-in boundary.  The reference (ChainUpZero/baby-plonk-rust) has no FFI of its own; the
 * entry points below are what a Rust `extern "C"` block in src/msm.rs / src/utils.rs / src/polynomial.rs /
 * src/setup.rs would bind (INTEGRATION.md shows those stubs).  Each entry names the reference interface it
 * replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain pointers and sizes only; no ownership transfer; every call returns BP_OK (0) or a negative code
 *     and never throws.  Where the reference panics (assert!, unwrap), the call returns an error instead and
 *     the Rust shim turns it back into a panic.
 *   - a bp_ctx is driven by one host thread (the reference is single-threaded); it owns its HIP stream(s),
 *     workspaces, SRS and circuit handles, so several contexts (one host thread each) may share a GPU and overlap
 *     their work.  Every entry point restores the calling thread's current HIP device before it returns.
 *   - multi-GPU, two ways:
 *       in one process   bp_init_multi(device_ids, n): ONE context drives n GPUs.  An SRS loaded or generated through it is
 *                        sharded by contiguous point range over the GPUs; bp_msm_g1 / bp_commit / bp_prove split the scalars
 *                        the same way, run the shards concurrently and add the partial sums -- the single-threaded Rust caller
 *                        of Setup::commit (src/setup.rs:32-37) uses all GPUs without knowing about them.  Batched host NTTs
 *                        (bp_ntt_fr with batch > 1) spread their independent columns over the GPUs.  Every GPU beyond the
 *                        first is driven by a persistent host thread of the library (uploads, waits, epilogues in parallel).
 *                        A list that names a device twice ({0,0}: what a one-GPU box can rehearse) makes a REHEARSAL group: its
 *                        members beyond the first take the GPU-to-GPU branches (hipMemcpyPeerAsync behind the leader's event)
 *                        exactly as members on other cards do.  STATUS: that is the only way those branches have run so far;
 *                        no run on distinct GPUs is recorded yet.
 *   - the library reads no environment variable (experiment knobs exist in the separate -DBP_EXPERIMENT build only).
 *       one process per GPU (torch.distributed / MPI launchers): every rank owns a point range in a plain bp_init context and
 *                        joins the library's own communicator (bp_comm_unique_id on rank 0, the host carries 128 bytes to the
 *                        others, bp_comm_init_rank everywhere).  bp_msm_g1_allgather then is the whole exchange under this ABI:
 *                        the rank's partial sums stay in HBM as a record, ONE ncclAllGather of the records over xGMI on the
 *                        context's stream, the slot-wise sum of the gathered records on the device, ONE 22-KB device-to-host
 *                        copy, host Horner; bp_ntt_columns_allgather gathers finished NTT columns in place.  A rank never skips
 *                        a collective (a local failure travels as a poisoned record / agreement word and every rank returns it),
 *                        and every wait behind a collective is bounded (bp_comm_set_timeout_ms): errors, not stalls.
 *                        (bp_msm_g1_blob_device + bp_msm_blobs_combine remain for hosts that bring their own collective.)
 *   - wire formats are the reference's own:
 *       scalar  fmt BP_FR_BYTES_LE : 32-byte little-endian canonical  (Scalar::to_bytes,  scalar.rs:292-304)
 *                                    a value >= q, as a scalar argument or as an element of a vector argument, is
 *                                    BP_ERR_BAD_SCALAR (Scalar::from_bytes rejects it, scalar.rs:264-288); for a vector the
 *                                    check runs on the device with the conversion (bp_poly_*, bp_grand_product, bp_ntt_fr on a
 *                                    single-device context), so the output buffer is unspecified after that error
 *               fmt BP_FR_MONT     : 4 x u64 Montgomery limbs          (Scalar::to_array,  scalar.rs:35-40)
 *       point   96-byte uncompressed affine, x||y big-endian, bit 6 of byte 0 = infinity
 *                                                                      (G1Affine::to_uncompressed, g1.rs:246-260)
 *       projective partial: 144 bytes = x|y|z, 6 x u64 Montgomery limbs each = the memory image of
 *               G1Projective (g1.rs:442-446); only used between our own ranks.
 *   - *_device variants take pointers to HBM (hipMalloc / torch CUDA tensors) and leave results there.
 */
#ifndef BP_MSM_NTT_H
#define BP_MSM_NTT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bp_ctx bp_ctx;

enum {
  BP_OK = 0,
  BP_ERR_INVALID_ARG = -1,   /* null pointer, bad format flag, bad handle */
  BP_ERR_NOT_POW2 = -2,      /* utils.rs:65,108   assert!(is_power_of_two(n)) */
  BP_ERR_BAD_POINT = -3,     /* non-canonical / off-curve / bad flags (g1.rs:273-322) */
  BP_ERR_BAD_SCALAR = -4,    /* 32-byte value >= q (scalar.rs:264-288) */
  BP_ERR_BASIS = -5,         /* polynomial.rs:35,48,53,319, setup.rs:34   assert_eq!(basis, ..) */
  BP_ERR_LENGTH = -6,        /* polynomial.rs:85-89,142-146   Lagrange operands of different length */
  BP_ERR_DIV_ZERO = -7,      /* polynomial.rs:347-348   division by the zero polynomial (unwrap on None) */
  BP_ERR_NO_DEVICE = -8,     /* no usable GPU / HIP runtime error at init */
  BP_ERR_HIP = -9,           /* HIP runtime error; bp_last_error() has the text */
  BP_ERR_TOO_LARGE = -10,    /* size beyond the supported range (NTT > 2^28, MSM >= 2^31 points) */
  BP_ERR_ASSERT = -11,       /* a protocol assert_eq! of the reference failed (prover.rs:319  z_n == 1) */
  BP_ERR_COMM = -12          /* an RCCL call failed, the communicator reported an asynchronous error, or a collective / ncclCommInitRank
                                did not finish within the bound of bp_comm_set_timeout_ms (the communicator is then aborted); text in bp_last_error */
};
enum { BP_FR_BYTES_LE = 0, BP_FR_MONT = 1 };
enum { BP_BASIS_LAGRANGE = 0, BP_BASIS_MONOMIAL = 1 };   /* polynomial.rs:8-11 */

/* ---- context ------------------------------------------------------------------------------------- */
int  bp_init(bp_ctx** out, int device_id);
/* One context over n_devices GPUs (`bp_init(out, device_ids, n_devices)`); device_ids[0] is the primary
 * device: polynomial operators, the prover's rounds and *_device pointers live there, MSMs and SRS storage span all of
 * them.  A device may be listed more than once (each listing is an independent shard; used to test the path on one GPU).
 * n_devices == 1 is the same as bp_init. */
int  bp_init_multi(bp_ctx** out, const int* device_ids, int n_devices);
/* number of shards of the context (1 for bp_init); device_ids, if not NULL, receives up to cap of their device ids */
int  bp_ctx_devices(bp_ctx* ctx, int* device_ids, int cap);
void bp_destroy(bp_ctx* ctx);
const char* bp_last_error(bp_ctx* ctx);            /* text of the last error on this ctx ("" if none) */
const char* bp_version(void);
/* Run all subsequent work of this ctx on an existing hipStream_t (e.g. torch's current stream). NULL = own stream.
 * Every entry point that reads or writes CALLER device memory (the *_device family) is ordered on that stream: work the caller
 * enqueued on the same stream before the call is seen, work enqueued after sees the call's results -- the blocking forms
 * additionally wait for the stream, the *_async forms do not.  On the context's own stream (the default) the caller must
 * have finished its pending work on those buffers before the call. */
int  bp_set_stream(bp_ctx* ctx, void* hip_stream);
int  bp_synchronize(bp_ctx* ctx);

/* ---- SRS: Setup.powers_of_x (src/setup.rs:7-10), resident in HBM ----------------------------------- */
/* Upload n points in the 96-byte encoding.  Replaces handing &self.powers_of_x to bucket_msm on every
 * commit (setup.rs:36): the SRS is immutable after construction, so it is uploaded once and cached.
 * Checks = G1Affine::from_uncompressed_unchecked + is_on_curve (g1.rs:273-322, 101-106): canonical coordinates, flag
 * bits, curve equation -> BP_ERR_BAD_POINT.  Subgroup membership (is_torsion_free, the extra check of the checked
 * decoder from_uncompressed) is NOT tested: an SRS comes from a trusted setup, as the reference's own Setup does. */
int  bp_srs_load(bp_ctx* ctx, const uint8_t* points96, size_t n, uint64_t* srs_handle);
/* The literal bucket_msm(points: &[G1Projective], ..) seam (src/msm.rs:76-81): n points as the in-memory image of
 * G1Projective (x | y | z, 6 x u64 Montgomery limbs each = 144 bytes, g1.rs:442-446), e.g. the Vec<G1Projective> of
 * Setup::powers_of_x handed over as a byte slice.  Normalised on the GPU (one shared inversion per 8 points, what
 * G1Projective::batch_normalize does on the host, g1.rs:806-839); z = 0 is the identity.  No curve check: the type
 * guarantees it (as G1Affine::from(&G1Projective) assumes). */
int  bp_srs_load_projective144(bp_ctx* ctx, const uint8_t* points144, size_t n, uint64_t* srs_handle);
/* A ceremony's SRS: n points in the 48-byte compressed encoding (G1Affine::to_compressed, g1.rs:221-244), decoded on the GPU.
 * checks = BP_SRS_CHECK_SUBGROUP: G1Affine::from_compressed (g1.rs:326-331); checks = 0: from_compressed_unchecked (g1.rs:337-390).
 * A record is rejected when its compression flag is clear, the masked x is >= p, the infinity flag is set with x != 0 or with the sort
 * flag, x^3 + 4 has no square root, or (checked) the point lies outside the prime-order subgroup (is_torsion_free, g1.rs:401-411).
 * y is chosen by lexicographically_largest() ^ sort flag; the identity is 0xc0 then zeros.  Any rejection is BP_ERR_BAD_POINT:
 * first_bad (may be NULL) receives the lowest failing global index, bp_last_error names it and the reason (encoding / not on the
 * curve / not in the subgroup), and no handle is created.  On success *first_bad = SIZE_MAX.  Sharded like bp_srs_load on
 * bp_init_multi contexts; n == 0 behaves as bp_srs_load with n == 0.  Unlike the reference (CtOption, constant time) the GPU code is
 * variable-time: SRS points are public. */
#define BP_SRS_CHECK_SUBGROUP 1u
int  bp_srs_load_compressed48(bp_ctx* ctx, const uint8_t* points48, size_t n, uint32_t checks, uint64_t* srs_handle, size_t* first_bad);
/* is_torsion_free (g1.rs:401-411) of points [first, first+n) of any SRS, on the GPU: what from_uncompressed adds to bp_srs_load's
 * checks.  BP_OK with *first_bad = SIZE_MAX, or BP_ERR_BAD_POINT with the lowest global index outside the subgroup in *first_bad
 * (may be NULL) and in bp_last_error. */
int  bp_srs_check_subgroup(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, size_t* first_bad);
/* The same seam as ONE call, nothing cached: result = sum_i scalars[i] * points[i] over min(n_points, n_scalars) pairs (the zip of
 * msm.rs:85), both operands in host memory.  Equivalent to bp_srs_load_projective144 + bp_msm_g1 + bp_srs_free, but the operands cross
 * PCIe in two pieces and the multiplication of the first runs while the second is uploaded and normalised, out of workspaces instead
 * of an SRS entry (from 2^17 pairs; below that, and on bp_init_multi contexts, it is the three calls): 8.3 against 8.9 ms at 2^20.  Statistics afterwards (bp_msm_last_stats): additions of all pieces,
 * times of the last piece. */
int  bp_msm_g1_projective144(bp_ctx* ctx, const uint8_t* points144, size_t n_points, const void* scalars, size_t n_scalars, int scalar_fmt,
                             uint8_t out96[96]);
/* Setup::generate_srs(powers, tau) (setup.rs:12-31): P_i = tau^i * G, generated on the GPU. tau: 32-byte LE. */
int  bp_srs_generate(bp_ctx* ctx, size_t powers, const uint8_t tau32[32], uint64_t* srs_handle);
/* Synthetic benchmark points P_i = (a + i*d) * G, generated on the GPU. */
int  bp_srs_generate_progression(bp_ctx* ctx, size_t n, const uint8_t a32[32], const uint8_t d32[32], uint64_t* srs_handle);
int  bp_srs_len(bp_ctx* ctx, uint64_t srs_handle, size_t* n);
/* Read points [first, first+n) back in the 96-byte encoding (G1Affine::to_uncompressed). */
int  bp_srs_export(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* points96);
/* The same points in the 48-byte compressed encoding (G1Affine::to_compressed, g1.rs:221-244), encoded on the GPU. */
int  bp_srs_export_compressed48(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* points48);
/* The same points as G1Projective memory images (z = 1, the identity as (0 : 1 : 0)): G1Projective::from(&G1Affine), g1.rs:176-190. */
int  bp_srs_export_projective144(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n, uint8_t* points144);
int  bp_srs_free(bp_ctx* ctx, uint64_t srs_handle);
/* Fixed-base window tables for an SRS that serves many commitments (Setup lives as long as the prover,
 * src/setup.rs:7-10): T[w][i] = 2^(window_bits * w) * P_i for every window w, affine, resident in HBM
 * (windows x srs_len x 128 bytes -- a 112-byte point per 128-byte cache line: 1.7 GB at 2^20 points, 28 GB at 2^24).  With tables every window of an
 * MSM feeds one shared bucket set, so the bucket reduction and the Horner epilogue shrink from `windows`
 * passes to one; results are the same group element.  From 21-bit windows the rows are R^w * P_i for a digit radix R that need not
 * be a power of two (12 windows of 22 bits cover 264 bits for 255-bit scalars: R = 0x288000 fills 1.33 M buckets instead of 2.1 M;
 * csrc/msm_digits.hpp) -- invisible at this boundary, same bytes out.  window_bits: 0 = chosen from srs_len (16 below 2^20 points, 20 -- thirteen
 * windows -- from 2^20 points, 22 from 2^24), BP_SRS_TABLES_OFF = drop the tables, else 4..24 (above 16 the bucket sort is partitioned).  MSMs shorter than 2^window_bits / 8 scalars keep
 * using the table-free path.  The reference has no counterpart (its MSM recomputes from the raw points).
 * Memory budget (hipMemGetInfo per device; the bytes of the tables this SRS holds now count as free): window_bits = 0 never fails
 * for lack of memory -- a width that does not fit beside what else lives on the device falls back to wider windows (fewer rows; only
 * widths an MSM over this SRS would use, 8 * srs_len >= 2^width) and then to no tables at all (bp_srs_table_info reports what was
 * built; results are the same bytes either way); an explicit width that does not fit returns BP_ERR_TOO_LARGE with the sizes in
 * bp_last_error() before anything is released or allocated: the SRS keeps the tables it had.  Any other window_bits is
 * BP_ERR_INVALID_ARG, and the SRS keeps its tables likewise. */
#define BP_SRS_TABLES_OFF 1u
int  bp_srs_precompute(bp_ctx* ctx, uint64_t srs_handle, uint32_t window_bits);
/* window_bits / windows / bytes of the tables of an SRS (all 0 without tables). */
int  bp_srs_table_info(bp_ctx* ctx, uint64_t srs_handle, uint32_t* window_bits, uint32_t* windows, uint64_t* bytes);
/* The Lagrange-basis SRS of a powers-of-tau SRS: for n = 2^log_n <= srs_len the new SRS holds L = i_ntt_381(P_0 .. P_{n-1}) taken in
 * G1 (utils.rs:106-129 with G1 additions and scalar multiplications in place of the Fr ones), i.e. L_i = [L_i(tau)] G for the Lagrange
 * polynomials over the n-th roots of unity -- computed on the GPU without tau, so it works for a ceremony file.  For every v of n
 * values, sum_i v_i L_i is the commitment of the polynomial whose evaluations are v: bp_commit* against the new handle take
 * BP_BASIS_LAGRANGE polynomials of exactly n values (BP_ERR_LENGTH otherwise; a Monomial polynomial is BP_ERR_BASIS), with no
 * inverse transform in front and with the column's small values visible to the MSM.  The new handle is an ordinary SRS of n points
 * (len, export, subgroup check, tables, MSM, free; sharded like any other on a bp_init_multi context); the source is untouched and
 * points beyond n are not read.  log_n <= 24 (BP_ERR_TOO_LARGE above); an unknown handle or 2^log_n > srs_len is
 * BP_ERR_INVALID_ARG; a source that is itself a Lagrange SRS is BP_ERR_BASIS. */
int  bp_srs_lagrange(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint64_t* lagrange_handle);
/* BP_BASIS_MONOMIAL and 0 for a loaded or generated SRS, BP_BASIS_LAGRANGE and its log_n for one made by bp_srs_lagrange.  Either
 * output pointer may be null. */
int  bp_srs_basis(bp_ctx* ctx, uint64_t srs_handle, int* basis, uint32_t* log_n);

/* ---- MSM: BucketMSM::bucket_msm(points, scalars, b, c) (src/msm.rs:76-118) ----------------------- */
/* sum_{i < min(n_scalars, srs_len - first)} s_i * P_{first+i}   (zip truncation of msm.rs:29).
 * The window parameters (b, c) of the reference are not taken: for b = 256 and c dividing 256 -- the only configuration
 * the reference calls it with (setup.rs:36: b = 256, c = 4) -- they do not change the group element.  (For other values
 * msm.rs:83,119-139 drops the low 256 - c*floor(b/c) bits of every scalar; that is not reproduced, and the mirrors of
 * BucketMSM::bucket_msm reject such (b, c).)
 * out96: affine result in the 96-byte encoding (identity = 0x40 then zeros). */
int  bp_msm_g1(bp_ctx* ctx, uint64_t srs_handle, const void* scalars, size_t n_scalars, int scalar_fmt,
               uint8_t out96[96]);
/* Same sum over the SRS slice starting at `first`, result as a 144-byte projective partial (multi-GPU:
 * each rank owns a point range; partials are all-gathered and added).  scalars_on_device != 0: `scalars`
 * points to HBM. */
int  bp_msm_g1_partial(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars,
                       int scalar_fmt, int scalars_on_device, uint8_t out144[144]);
/* One process per GPU: the same sum as bp_msm_g1_partial, left in HBM as an opaque BP_MSM_BLOB_BYTES record at d_blob (the
 * per-window / per-bit-plane partial sums of this rank, not yet combined).  The caller all-gathers the records of all
 * ranks on the device (RCCL) and hands the gathered host copy to bp_msm_blobs_combine: one collective and one
 * device-to-host copy per MSM, no host hop before the exchange.  The record is complete when the call returns (it is
 * written on the context's own stream, which the call waits for); work the caller still has pending on d_blob on another
 * stream -- e.g. the zero fill of a freshly allocated torch tensor -- must have finished before the call. */
#define BP_MSM_BLOB_BYTES 22592u      /* 64-byte header + 128 accumulator slots of 176 bytes */
int  bp_msm_g1_blob_device(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                           int scalars_on_device, void* d_blob);
/* The same, STREAM-ORDERED: enqueued on the context's stream and not waited for.  With bp_set_stream(the caller's stream) the
 * record is written in that stream's order: behind whatever the caller enqueued on d_blob or the scalars before (a zero fill,
 * a producer kernel), in front of whatever it enqueues next (the RCCL all-gather of dist.ShardedMsm) -- no host wait, and
 * ordering is a property of the call, not of prose.  Errors that need the result (a canonical-bytes scalar >= q) travel in
 * the record's header and surface in bp_msm_blobs_combine.  bp_msm_last_stats reads the timing once the stream has passed it.
 * Host scalars (scalars_on_device == 0) are copied by a stream-ordered hipMemcpyAsync: from pageable memory the runtime has
 * staged them when the call returns, from PINNED memory (hipHostMalloc, a torch pinned tensor) the DMA reads them later --
 * the buffer must stay valid and unchanged until the stream has passed the call (bp_synchronize, or an event of the caller's). */
int  bp_msm_g1_blob_device_async(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                                 int scalars_on_device, void* d_blob);
/* Optional device-side pre-sum of the gathered records (n_blobs of them in HBM, BP_MSM_BLOB_BYTES apart): records of equal
 * window layout -- the normal case -- are added slot by slot on the GPU into ONE record at d_out_blob, so only 22 KB cross to
 * the host and the host does one Horner pass.  If the layouts differ the output record is marked invalid (bp_msm_blobs_combine
 * rejects it with BP_ERR_INVALID_ARG) and the caller combines the gathered records on the host instead. */
int  bp_msm_blobs_sum_device(bp_ctx* ctx, const void* d_blobs, size_t n_blobs, void* d_out_blob);
/* The same, stream-ordered (enqueued on the context's stream, not waited for). */
int  bp_msm_blobs_sum_device_async(bp_ctx* ctx, const void* d_blobs, size_t n_blobs, void* d_out_blob);
/* Host-side: combine n_blobs records (host memory, BP_MSM_BLOB_BYTES apart) into the affine result.  Records with the
 * same window layout are added slot by slot before the one Horner pass (msm.rs:107-115). */
int  bp_msm_blobs_combine(const void* blobs, size_t n_blobs, uint8_t out96[96]);
/* Host-side, no GPU: the scalars that BucketMSM::bucket_msm(points, scalars, b, c) effectively multiplies the points by, for ANY
 * (b, c).  The reference walks k = floor(b / c) windows of c bits over the 256-bit big-endian image of the scalar, most
 * significant first (msm.rs:83, 119-139), so it uses the top k*c bits only: result = sum_i (K_i >> (256 - k*c)) * P_i.  For its
 * one call site (b = 256, c = 4, setup.rs:36) and whenever c divides 256 = b the shift is zero.  out_le32 receives n 32-byte
 * little-endian canonical values (feed them to bp_msm_g1 with BP_FR_BYTES_LE).  BP_ERR_INVALID_ARG where the reference panics:
 * c = 0 (division by zero), k = 0 (t_points[0], msm.rs:105), k*c > 256 (bit slice out of range, msm.rs:132), c > 63
 * (the 1 << c bucket vector, msm.rs:24). */
int  bp_msm_window_scalars(const void* scalars, size_t n, int scalar_fmt, size_t b, size_t c, void* out_le32);
/* Host-side: add n projective partials (complete addition, g1.rs:670-712) and normalise (g1.rs:49-63). */
int  bp_g1_sum_partials(const uint8_t* partials144, size_t n, uint8_t out96[96]);
/* Host-side conversions of single points (for the Rust shim's G1Projective <-> bytes plumbing). */
int  bp_g1_partial_to_bytes96(const uint8_t in144[144], uint8_t out96[96]);
int  bp_g1_bytes96_to_partial(const uint8_t in96[96], uint8_t out144[144]);
/* G1Affine::to_compressed (g1.rs:221-244): the 48-byte encoding the transcript absorbs (transcript.rs:66-69) and
 * bp_prove emits; host-side, no GPU. */
int  bp_g1_bytes96_to_compressed48(const uint8_t in96[96], uint8_t out48[48]);
/* HIP-event duration of the bucket-accumulation kernel of the last MSM on this ctx, and its adds. */
int  bp_msm_last_stats(bp_ctx* ctx, float* accumulate_ms, float* total_device_ms, uint64_t* mixed_adds,
                       uint32_t* window_bits);
/* The same per member of a bp_init_multi context (member 0 .. bp_ctx_devices() - 1; a plain context has member 0 only), plus
 * the time of the member's scalar upload when the last MSM took host scalars (0 otherwise): the split of one
 * Setup::commit(&Polynomial) (setup.rs:32-37) over the GPUs into PCIe time and compute time.  Any pointer may be null. */
int  bp_msm_last_member_stats(bp_ctx* ctx, int member, float* upload_ms, float* accumulate_ms, float* total_device_ms,
                              uint64_t* mixed_adds);
/* Which path the last MSM pipeline enqueued on a member's context took (member as in bp_msm_last_member_stats), twelve words:
 * J (scalar vectors in the pipeline), c, W (windows), radix (live buckets of a radix-R width, else 0), sort (1 two-level, 2 partition),
 * pb (partition bits), packed (one-word records), flat (flat write-out), wide8 (1 024-scalar slices of two-word records), fixup
 * (0 per bucket, 1 per chunk edge), n_wide (tree levels run one addition per lane), chunk (entries per accumulation lane).  Host
 * words stored at launch time: nothing is timed, waited for or read from the device; an empty MSM launches nothing and leaves them. */
int  bp_msm_last_path(bp_ctx* ctx, int member, uint32_t out[12]);
/* 1 when the last MSM on this ctx went through fixed-base tables, 0 when not, negative on error. */
int  bp_msm_last_used_tables(bp_ctx* ctx);

/* ---- one process per GPU: the collective under the boundary (SURVEY.md 8b "bp_ctx owns ... the RCCL comm", 8e) ------------------
 * The reference is one thread on one CPU (prover.rs has no notion of ranks); a Rust host that runs one process per GPU calls these
 * instead of bringing its own RCCL binding.  The library is linked against librccl; every collective is enqueued on the context's
 * stream between the library's own kernels.  Communicators belong to plain bp_init contexts (a bp_init_multi context combines its
 * shards itself).  Exercised on the build pool's one-GPU boxes with worlds of ONE rank only (tests/test_gpu_dist.py); no multi-GPU
 * run exists yet, and no number for a world > 1 is claimed.
 * bp_comm_unique_id: rank 0 makes the 128-byte id (ncclGetUniqueId); the host carries it to the other ranks by whatever means it
 * has (a file, a socket, MPI).  bp_comm_init_rank: every rank, same id (ncclCommInitRank; collective -- returns when all `world`
 * ranks have called it; it allocates every buffer the later collectives need and ends with a 32-byte agreement all-gather in
 * which the ranks compare world and record size).  bp_comm_info: rank / world of the context's communicator (world = 0 without one).
 * Failure semantics -- the reference panics, it never blocks (src/setup.rs:34, src/utils.rs:65,108), and neither does a collective here:
 *   - a rank that fails locally in front of a collective still JOINS it and says so inside it (a poisoned MSM record; the agreement
 *     word of bp_ntt_columns_allgather); every rank of the communicator then returns that rank's error code;
 *   - every host wait behind a collective polls the stream and ncclCommGetAsyncError and gives up after the bound of
 *     bp_comm_set_timeout_ms (milliseconds; default 120 000; 0 = wait for ever): the communicator is aborted (ncclCommAbort),
 *     bp_comm_info reports world 0, the call returns BP_ERR_COMM; a new communicator may be created afterwards;
 *   - ncclCommInitRank runs on a helper thread under the same bound; when it expires (a rank never arrived) the call returns
 *     BP_ERR_COMM, the helper stays parked inside RCCL until the process ends and this context refuses further communicators.
 * bp_comm_stats: collectives this context has enqueued so far (agreement all-gathers included) and the bound in force. */
#define BP_COMM_ID_BYTES 128
int  bp_comm_unique_id(uint8_t id[128]);
int  bp_comm_init_rank(bp_ctx* ctx, const uint8_t id[128], int rank, int world);
int  bp_comm_info(bp_ctx* ctx, int* rank, int* world);
int  bp_comm_set_timeout_ms(bp_ctx* ctx, uint32_t ms);
int  bp_comm_stats(bp_ctx* ctx, uint64_t* collectives, uint32_t* timeout_ms);
int  bp_comm_destroy(bp_ctx* ctx);
/* Setup::commit / BucketMSM::bucket_msm over ALL ranks (src/setup.rs:32-37 -> src/msm.rs:76-118): every rank passes the scalars of
 * ITS point range (srs_handle = the rank's shard, `first` inside it, zip truncation as bp_msm_g1_partial) and every rank receives
 * the same 96 bytes: sum over all ranks' (point, scalar) pairs.  Inside: the rank's bit planes stay in HBM as a BP_MSM_BLOB_BYTES
 * record -> ONE ncclAllGather of the records over xGMI -> slot-wise sum of the gathered records on the device -> ONE 22-KB
 * device-to-host copy -> host Horner (msm.rs:107-115) + normalisation.  One host wait per call.  Collective: every rank of the
 * communicator must call it (an empty range is fine: n_scalars = 0).  A rank whose own part fails (unknown handle, `first` beyond
 * its shard, out of memory, a scalar >= q) still takes part: its record carries the error and EVERY rank returns that code. */
int  bp_msm_g1_allgather(bp_ctx* ctx, uint64_t srs_handle, size_t first, const void* scalars, size_t n_scalars, int scalar_fmt,
                         int scalars_on_device, uint8_t out96[96]);
/* GPU time of the last bp_msm_g1_allgather from "this rank's record complete" to "gathered, summed and copied" (HIP events). */
int  bp_comm_last_exchange_ms(bp_ctx* ctx, float* ms);
/* NTT by independent columns (Polynomial::ntt / i_ntt on separate polynomials, src/polynomial.rs:47-55): d_columns holds
 * world x columns_per_rank columns of 2^log_n Montgomery elements in HBM, rank r's finished columns in block r (this rank's block
 * filled by its own bp_ntt_fr_device calls on this context); ONE in-place ncclAllGather leaves every column on every rank.  A 32-byte
 * agreement all-gather goes first (status, log_n, columns_per_rank of every rank): a rank with bad arguments, or ranks that disagree
 * on the shape, make every rank return the same error before any column moves.  log_n <= 28. */
int  bp_ntt_columns_allgather(bp_ctx* ctx, void* d_columns, uint32_t log_n, size_t columns_per_rank);

/* ---- DFT: ntt_381 / i_ntt_381 (src/utils.rs:63-81, 106-129) --------------------------------------- */
/* In-place natural-order transform of length 2^log_n on `batch` vectors, vector b at data + b*stride
 * elements (32 bytes each).  inverse != 0 includes the 1/N scaling (utils.rs:126). */
int  bp_ntt_fr(bp_ctx* ctx, void* data, uint32_t log_n, int inverse, int scalar_fmt, size_t batch, size_t stride);
/* Same on HBM-resident Montgomery data. */
int  bp_ntt_fr_device(bp_ctx* ctx, void* d_data, uint32_t log_n, int inverse, size_t batch, size_t stride);
/* Same, enqueued only: returns once the kernels are on the context's stream (the one given to bp_set_stream, or the context's own);
 * bp_synchronize or any blocking entry point of this context waits for them.  d_data must stay valid until then. */
int  bp_ntt_fr_device_async(bp_ctx* ctx, void* d_data, uint32_t log_n, int inverse, size_t batch, size_t stride);
/* HIP-event duration of all kernels of the last bp_ntt_fr_device / _async call (0 while an enqueued one is still running). */
int  bp_ntt_last_stats(bp_ctx* ctx, float* device_ms, uint32_t* passes);
/* Group contexts (bp_init_multi) and host data: batch > 1 deals the columns round-robin to the members (option i);
 * ONE transform of 2^22 elements or more (BP_NTT_GROUP_SPLIT_FROM) is cut over the members (option ii): each uploads a slice
 * of the columns of the first pass over its own PCIe link, the members swap blocks of the intermediate buffer (peer copies),
 * run the remaining passes on their share and download their outputs.  A member count that is not 2, 4 or 8, or a shape
 * that does not divide, runs on the first device.  Number of members that took part in the last bp_ntt_fr call: */
int  bp_ntt_last_members(bp_ctx* ctx);
/* root_of_unity(n) (utils.rs:39-43) and roots_of_unity(n) (utils.rs:45-52), output in scalar_fmt. */
int  bp_root_of_unity(uint64_t group_order, int scalar_fmt, uint8_t out32[32]);
int  bp_roots_of_unity(bp_ctx* ctx, uint64_t group_order, int scalar_fmt, void* out);

/* Host-side format conversion of n scalars between BP_FR_BYTES_LE and BP_FR_MONT (Scalar::from_bytes / to_bytes,
 * scalar.rs:264-304); returns BP_ERR_BAD_SCALAR for a canonical input >= q.  in == out is allowed. */
int  bp_fr_convert(const void* in, size_t n, int from_fmt, int to_fmt, void* out);

/* Synthetic benchmark scalars written straight into HBM (Montgomery limbs): element i = Scalar::from_bytes_wide
 * (scalar.rs:308-339) of 64 bytes of a SplitMix64 stream. Not in the reference. */
int  bp_fr_synthetic_device(bp_ctx* ctx, void* d_out, size_t n, uint64_t seed);

/* ---- Polynomial (src/polynomial.rs:14-380); values are n x 32-byte scalars in scalar_fmt ---------- */
/* coeffs_evaluate (polynomial.rs:34-45); asserts Monomial basis. */
int  bp_poly_evaluate(bp_ctx* ctx, const void* coeffs, size_t n, int basis, const void* x32, int scalar_fmt,
                      void* out32);
/* impl Add/Sub for Polynomial (polynomial.rs:76-117,134-174). out needs max(na,nb) slots; *n_out = length. */
int  bp_poly_add(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt,
                 void* out, size_t* n_out);
int  bp_poly_sub(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt,
                 void* out, size_t* n_out);
/* impl Add<Scalar>/Sub<Scalar>/Mul<Scalar> (polynomial.rs:57-74,119-132,176-187), including the reference's
 * Lagrange-basis Sub<Scalar> quirk (it adds, :126-128). op: 0 add, 1 sub, 2 mul. */
int  bp_poly_scalar_op(bp_ctx* ctx, const void* a, size_t n, int basis, const void* s32, int op, int scalar_fmt,
                       void* out);
/* impl Mul for Polynomial, Monomial basis (polynomial.rs:240-273): out has na+nb-1 coefficients. */
int  bp_poly_mul(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt,
                 void* out, size_t* n_out);
/* impl Div for Polynomial (polynomial.rs:314-380): quotient only, exactly as the reference produces it
 * (zero quotient coefficients are squeezed out).  out needs na slots. */
int  bp_poly_div(bp_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, int basis, int scalar_fmt,
                 void* out, size_t* n_out);
/* Round-2 permutation grand product (prover.rs:279-319), "next" row f2 of SURVEY.md section 8.  Six Lagrange-basis
 * columns of n values (witness a, b, c and sigma s1, s2, s3), challenges beta, gamma and coset shifts k1, k2
 * (prover.rs:99-100: 2 and 3) as 32-byte scalars in scalar_fmt.  z_out receives z_0 .. z_{n-1} (z_0 = 1).
 * BP_ERR_DIV_ZERO where a denominator is zero (invert().unwrap()), BP_ERR_ASSERT where z_n != 1 (:319).
 * One batched inversion for all 3n denominators: z_i = prefix(num)_i * suffix(den)_i / prod(den). */
int  bp_grand_product(bp_ctx* ctx, const void* a, const void* b, const void* c, const void* s1, const void* s2, const void* s3,
                      size_t n, const void* beta32, const void* gamma32, const void* k1_32, const void* k2_32, int scalar_fmt,
                      void* z_out);

/* ---- the same operators on HBM-resident data (Montgomery limbs) -------------------
 * d_* are device pointers (hipMalloc / torch CUDA tensors); scalars and results of O(1) size stay on the host.
 * Semantics, length rules, quirks and error codes are those of the host-pointer entry points above.
 * add, sub and scalar_op are element-wise: d_out may be d_a (or d_b) itself, in place; any other overlap, and any overlap in the
 * other entry points, is not allowed. */
int  bp_poly_add_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out);
int  bp_poly_sub_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out);
int  bp_poly_scalar_op_device(bp_ctx* ctx, const void* d_a, size_t n, int basis, const void* s32_mont, int op, void* d_out);
int  bp_poly_mul_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out);
int  bp_poly_div_device(bp_ctx* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, int basis, void* d_out, size_t* n_out);
int  bp_poly_evaluate_device(bp_ctx* ctx, const void* d_coeffs, size_t n, int basis, const void* x32_mont, void* out32_mont);
/* out[i] = a[i] * w^i, i.e. p(x) -> p(w x)  (prover.rs:661-674 monomial_z_to_z_omega) */
int  bp_poly_scale_powers_device(bp_ctx* ctx, const void* d_a, size_t n, const void* w32_mont, void* d_out);
/* Which kernels the last bp_poly_div / bp_poly_div_device of this context ran (no timing, nothing waited for).  div_path: 0 general
 * long division, or for a binomial divisor b0 + bm x^m with chunks = ceil(ceil(nq / m) / 32) chunks per chain: 1 one chunk (no carry),
 * 2 carries by one lane per chain, 3 by one workgroup per chain, 4 by `segments` workgroups per chain.  chunks is 0 on the general
 * path, segments is 0 on every path but 4.  Any pointer may be null. */
int  bp_poly_last_stats(bp_ctx* ctx, uint32_t* div_path, uint64_t* chunks, uint32_t* segments);
int  bp_roots_of_unity_device(bp_ctx* ctx, uint64_t group_order, void* d_out);
int  bp_grand_product_device(bp_ctx* ctx, const void* d_a, const void* d_b, const void* d_c, const void* d_s1, const void* d_s2,
                             const void* d_s3, size_t n, const void* beta32, const void* gamma32, const void* k1_32,
                             const void* k2_32, void* d_z);
int  bp_commit_device(bp_ctx* ctx, uint64_t srs_handle, const void* d_coeffs, size_t n, int basis, uint8_t out96[96]);
/* `count` commitments against one SRS (prover.rs:249-251, 483-485, 640-641 commit two or three polynomials in a row): polynomial i
 * = n[i] Montgomery coefficients in HBM at d_coeffs[i]; out96 receives count x 96 bytes.  The pipelines run together. */
int  bp_commit_many_device(bp_ctx* ctx, uint64_t srs_handle, const void* const* d_coeffs, const size_t* n, size_t count, int basis,
                           uint8_t* out96);

/* Setup::commit (setup.rs:32-37): asserts Monomial basis, MSM of the coefficients against the SRS.  The three commit entry points
 * ask one rule: the polynomial's basis must be the SRS's (bp_srs_basis) -- Monomial for every loaded or generated SRS, as in the
 * reference; Lagrange, with exactly srs_len values, for an SRS made by bp_srs_lagrange. */
int  bp_commit(bp_ctx* ctx, uint64_t srs_handle, const void* coeffs, size_t n, int basis, int scalar_fmt,
               uint8_t out96[96]);

/* ---- Prover::prove (src/prover.rs:64-175; rounds :177-647) -- SURVEY.md 8f "next" rows 1-3 ------------------ */
/* Preprocessed circuit = CommonPreprocessedInput (src/program.rs:34-50): the eight Lagrange columns
 * QL QR QM QO QC S1 S2 S3 (in this order) of a 2^log_n-row circuit, log_n >= 3.  Uploaded once and kept in HBM
 * with the forms the reference re-derives inside every proof (coefficient forms, prover.rs:379-386).
 * columns_on_device != 0: the eight pointers are HBM addresses of Montgomery data. */
int  bp_circuit_load(bp_ctx* ctx, uint32_t log_n, const void* const columns[8], int scalar_fmt, int columns_on_device,
                     uint64_t* circuit_handle);
int  bp_circuit_free(bp_ctx* ctx, uint64_t circuit_handle);
/* The verifier's preprocessing (src/verifier.rs:61-68: i_ntt + Setup::commit of each column): commitments to
 * QL QR QM QO QC S1 S2 S3 in that order, 8 x 96 bytes (uncompressed affine), from the coefficient forms already in HBM. */
int  bp_circuit_commitments(bp_ctx* ctx, uint64_t srs_handle, uint64_t circuit_handle, uint8_t out768[768]);
/* Program::make_s_polynomials (src/program.rs:76-147) for circuits of any size: the reference labels every cell with
 * roots_of_unity(group_order)[row] recomputed per cell (utils.rs:29-36), i.e. O(n^2) field work; this is the same map in
 * O(n log n) on the host (no GPU needed).  wire_ids: 3 * 2^log_n variable ids, row-major, columns L R O inside a row;
 * 0 = empty wire (the reference's None), equal ids = the same variable name.  Empty rows after the constraints are rows
 * of zeros.  Cells of one variable form a cycle in row-major order and the NEXT cell of the cycle receives THIS cell's
 * label column * w^row, columns numbered 1 2 3 (program.rs:126-137).  s1 s2 s3: 2^log_n Montgomery scalars each, host. */
int  bp_make_s_polynomials(uint32_t log_n, const uint32_t* wire_ids, void* s1, void* s2, void* s3);
/* A circuit from what follows the reference's parser (assembly.rs, program.rs): per row five selector values and three variable
 * ids.  selectors: QL QR QM QO QC, 2^log_n scalars each; wire_ids: as bp_make_s_polynomials takes them (3 * 2^log_n ids, row-major,
 * columns L R O, 0 = empty wire, any uint32).  S1 S2 S3 are built on the GPU by the map of program.rs:76-147 -- a stable 8-bit
 * radix sort of the cells by id (as many passes as the largest id needs, 0..4) and one link pass -- and are the columns
 * bp_make_s_polynomials returns, byte for byte.  n_public <= 2^log_n: rows 0 .. n_public-1 are the public rows and the public
 * variable of row i is its L wire (prover.rs:114-127).  inputs_on_device != 0: the five selector pointers and wire_ids are HBM
 * addresses, the selectors Montgomery.  BP_ERR_BAD_SCALAR: a BP_FR_BYTES_LE selector >= q.  The handle is a circuit handle like
 * bp_circuit_load's (bp_prove, bp_circuit_commitments, the checks, group contexts, bp_circuit_free); it also keeps the wire ids in
 * HBM (12 bytes per row) for the two assignment calls below, and the cell map the link pass wrote, so bp_circuit_check_sigma /
 * _witness never decode such a circuit (decode time 0, both counts 0 and both positions absent: the cycles are a permutation
 * by construction). */
int  bp_circuit_load_wires(bp_ctx* ctx, uint32_t log_n, const void* const selectors[5], const uint32_t* wire_ids, size_t n_public,
                           int scalar_fmt, int inputs_on_device, uint64_t* circuit_handle);
/* HIP-event milliseconds of the last bp_circuit_load_wires on this ctx: upload + conversion of the inputs, the largest id (with its
 * read-back), the sort, the table of roots + the link pass, the derived forms every circuit handle holds (bp_circuit_load's work). */
int  bp_circuit_load_wires_last_stats(bp_ctx* ctx, float stage_ms[5]);
/* The eight Lagrange columns QL QR QM QO QC S1 S2 S3 of any circuit handle, 2^log_n scalars each, to host memory; a NULL entry of
 * `columns` skips that column.  How a verifier-side host sees the sigma bp_circuit_load_wires built. */
int  bp_circuit_export_columns(bp_ctx* ctx, uint64_t circuit_handle, int scalar_fmt, void* const columns[8]);
/* A witness from one value per variable: values[id] for id < n_values (slot 0 is never read: an empty wire is zero; device values
 * must be Montgomery).  Writes 2^log_n Montgomery scalars per column into caller-owned HBM: a[row] = values[wire_ids[3 row]],
 * b and c likewise, PI[row] = -values[wire_ids[3 row]] for row < n_public and zero elsewhere (prover.rs:120-127); d_pi may be NULL.
 * Copy constraints hold by construction.  BP_ERR_LENGTH: a wire id >= n_values (bp_last_error names the lowest such cell; the
 * columns are unspecified then); BP_ERR_BAD_SCALAR: a BP_FR_BYTES_LE value >= q; BP_ERR_INVALID_ARG: a handle of bp_circuit_load,
 * which holds no wire ids.  Blocking. */
int  bp_circuit_assign_device(bp_ctx* ctx, uint64_t circuit_handle, const void* values, size_t n_values, int scalar_fmt,
                              int values_on_device, void* d_a, void* d_b, void* d_c, void* d_pi);
/* bp_prove from the same value array: the gather of bp_circuit_assign_device into the prover's own workspace, then the proof.
 * Same bytes and same errors as bp_prove on the expanded columns. */
int  bp_prove_assignment(bp_ctx* ctx, uint64_t srs_handle, uint64_t circuit_handle, const void* values, size_t n_values,
                         int scalar_fmt, int values_on_device, const uint8_t blinders[352], uint8_t proof[624]);
/* One proof.  a, b, c: the witness as the three Lagrange wire columns the reference builds at prover.rs:186-227;
 * public_input: the Lagrange column of prover.rs:114-127 (-x_i in the first rows, zero elsewhere), NULL = all zero;
 * 2^log_n scalars each.  blinders: b1..b11 of prover.rs:110 as 11 x 32 canonical little-endian bytes -- an input here
 * (prove_with_blinding), because the reference draws them from thread_rng and is therefore not reproducible.
 * The SRS should hold 2^log_n + 6 points (verify_proof_test.rs:16); a shorter one truncates the commitments the way
 * Setup::commit's zip does (msm.rs:29), as in the reference.  Challenges come from the reference's transcript
 * (src/transcript.rs:4-86; merlin 3.0.0 restated on the host).
 * proof: 9 x 48-byte compressed G1 points in Proof field order (verifier.rs:23-40: a_1 b_1 c_1 z_1 t_lo_1 t_mid_1
 * t_hi_1 w_zeta_1 w_zeta_omega_1), then a_bar b_bar c_bar s1_bar s2_bar z_omega_bar as 32-byte little-endian.
 * Errors mirror the reference's panics: BP_ERR_ASSERT for z_n != 1 (prover.rs:319) and r(zeta) != 0 (:615), i.e. a
 * witness that does not satisfy the circuit; BP_ERR_DIV_ZERO for a zero permutation denominator. */
int  bp_prove(bp_ctx* ctx, uint64_t srs_handle, uint64_t circuit_handle, const void* a, const void* b, const void* c,
              const void* public_input, int scalar_fmt, int witness_on_device, const uint8_t blinders[352],
              uint8_t proof[624]);
/* Host wall-clock milliseconds of rounds 1..5 and of the whole last bp_prove on this ctx. */
int  bp_prove_last_stats(bp_ctx* ctx, float round_ms[5], float* total_ms);
/* Where a witness fails its circuit.  The reference panics at prover.rs:319 (z_n != 1) and :615 (r(zeta) != 0) and bp_prove
 * answers BP_ERR_ASSERT there, after most of a proof's work and without a position; these two calls name the row and the cell,
 * from the eight Lagrange columns the circuit handle already holds in HBM.  Cells are numbered 3 * row + col (col 0 1 2 = A B C,
 * the numbering of bp_make_s_polynomials' wire_ids); an absent position is UINT64_MAX.  Blocking, ordered on the context's stream;
 * a group context (bp_init_multi) runs them on its first device.  A rejected call leaves `report` untouched.
 * Is (S1, S2, S3) a permutation of the 3 * 2^log_n cells?  Every value is decoded back from its label (col + 1) w^row
 * (program.rs:126-137) to the cell it names: report[0] = cells whose value is no cell label, report[1] = the lowest such cell,
 * report[2] = cells that are the target of != 1 cells, report[3] = the lowest such cell.  All counts 0 <=> sigma is a
 * permutation.  The decode runs on the first check of a circuit (either call) and stays with the handle until bp_circuit_free:
 * 12 bytes per row. */
int  bp_circuit_check_sigma(bp_ctx* ctx, uint64_t circuit_handle, uint64_t report[4]);
/* a, b, c, public_input, scalar_fmt, witness_on_device: as bp_prove takes them (a device witness is read in place).
 * report[0] = rows whose gate equation ql a + qr b + qm a b + qo c + PI + qc (prover.rs:370-376) is not zero, report[1] = the
 * lowest such row; report[2] = cells u whose value differs from the value at sigma(u), the cell S names at u, report[3] = the
 * lowest such u, report[4] = its sigma(u).  BP_OK means the check ran; the witness satisfies the circuit iff report[0] ==
 * report[2] == 0, and bp_prove answers BP_ERR_ASSERT exactly when it does not.  Values are compared as the Montgomery limbs
 * they are.  BP_ERR_BAD_SCALAR: a BP_FR_BYTES_LE value >= q.  BP_ERR_INVALID_ARG on a circuit whose sigma is no permutation
 * (the copy comparison means nothing then): bp_last_error names bp_circuit_check_sigma and the lowest bad cell. */
int  bp_circuit_check_witness(bp_ctx* ctx, uint64_t circuit_handle, const void* a, const void* b, const void* c,
                              const void* public_input, int scalar_fmt, int witness_on_device, uint64_t report[5]);
/* HIP-event milliseconds of the last of the two calls above on this ctx: the sigma decode (0 when the circuit already had it),
 * upload + conversion of a host witness, the check kernel. */
int  bp_circuit_check_last_stats(bp_ctx* ctx, float stage_ms[3]);
/* merlin conformance vector: Transcript::new("test protocol"), append_message("some label", "some data"),
 * challenge_bytes("challenge", 32) -- lets a binding check the host transcript without a GPU. */
int  bp_transcript_test_vector(uint8_t out32[32]);

/* ---- Verifier::verify (src/verifier.rs:80-209) for a batch, up to the two pairings ------------------------------ */
/* Verifier::compute_challengs (verifier.rs:193-209) for m proofs in the 624-byte encoding of bp_prove; host-side, no GPU.
 * out: m x 6 scalars in scalar_fmt, order beta gamma alpha zeta nu mu.  The transcript absorbs the 48 compressed bytes of every
 * point and the 32 little-endian bytes of every evaluation as they stand in the record (transcript.rs:66-69, 83-85); points are not
 * decoded here.  An evaluation >= q (Scalar::from_bytes, scalar.rs:264-288) is BP_ERR_BAD_SCALAR with the lowest such record in
 * *first_bad (may be NULL; SIZE_MAX on success).  m == 0: BP_OK. */
int  bp_plonk_challenges(const uint8_t* proofs624, size_t m, int scalar_fmt, void* out, size_t* first_bad);
/* Verifier::verify (verifier.rs:80-192) up to, and without, the two pairings, for m proofs of ONE circuit.
 * out192 = A || B (96-byte affine each, the identity as 0x40 then zeros) with
 *   A = sum_j rho_j (W_zeta_j + mu_j W_zeta_omega_j)
 *   B = sum_j rho_j (zeta_j W_zeta_j + mu_j zeta_j omega W_zeta_omega_j + F_j - E_j)          (verifier.rs:187-191)
 * The batch is valid iff pairing(A, x_2) == pairing(B, G2Affine::generator()) (up to the 2^-128 of the weights); the pairings stay
 * with the host (bls12_381::pairing).  bp_verify_reduce does not decide validity.
 *   log_n          group order n = 2^log_n, 3 <= log_n <= 28; omega = root_of_unity(n); k1 = 2, k2 = 3 (verifier.rs:76-77, 89).
 *   vk768          the eight commitments in the order bp_circuit_commitments writes them (QL QR QM QO QC S1 S2 S3; verifier.rs:61-68),
 *                  checked like bp_srs_load (canonical, flags, on the curve -> BP_ERR_BAD_POINT), not subgroup-checked: the verifier
 *                  computed them itself.
 *   proofs624      m records of bp_prove's output.  Each of the 9 points goes through the CHECKED decoder (G1Affine::from_compressed,
 *                  g1.rs:326-331: encoding, curve, subgroup; the identity 0xc0 00.. is a valid point); each of the 6 evaluations must
 *                  be < q.  BP_ERR_BAD_POINT / BP_ERR_BAD_SCALAR with *first_bad (may be NULL) = the lowest failing proof index -- a
 *                  bad point wins over a bad scalar only if its proof index is lower or equal -- bp_last_error names proof, field and
 *                  reason, out192 is left untouched.  On success *first_bad = SIZE_MAX.
 *   public_inputs  m x n_public scalars in scalar_fmt, row j = the vector handed to verify() for proof j (verifier.rs:99-104: negated,
 *                  zero-padded to n).  n_public may be 0 (the pointer is then ignored); n_public > n is BP_ERR_LENGTH.  PI(zeta) and
 *                  L_1(zeta) (verifier.rs:91-104) equal what i_ntt + coeffs_evaluate return for EVERY zeta, also where zeta^n = 1 (the
 *                  value is then [zeta == omega^i]); O(n_public) products and one inversion per proof.
 *   weights        m scalars rho_j in scalar_fmt, drawn by the caller AFTER it has seen the proofs, 128 bits of entropy or more each
 *                  (the reference draws its randomness with thread_rng on the host, prover.rs:108-110).  NULL means rho_j = 1 and is
 *                  accepted for m <= 1 only (BP_ERR_INVALID_ARG otherwise); with m == 1 and NULL the outputs are exactly the two
 *                  G1Affine arguments of verifier.rs:187-191.
 *   challenges     NULL = derived on the device from the proof bytes (verifier.rs:193-209).  Otherwise m x 6 scalars in scalar_fmt,
 *                  order as bp_plonk_challenges, used instead (a host with another transcript).
 * Canonical-bytes public inputs, weights and challenges >= q are BP_ERR_BAD_SCALAR with the proof index in *first_bad.
 * m == 0: BP_OK, A = B = identity.  9 m + 9 >= 2^31: BP_ERR_TOO_LARGE.  Null pointers, bad format, log_n out of range:
 * BP_ERR_INVALID_ARG.  A bp_init_multi context runs the batch on its primary device.  Blocking; ordered on the context's stream. */
int  bp_verify_reduce(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m,
                      const void* public_inputs, size_t n_public, const void* weights, const void* challenges,
                      int scalar_fmt, uint8_t out192[192], size_t* first_bad);
/* The same reduction per SEGMENT of the batch: segment s covers the proofs [s * segment, min(m, (s + 1) * segment)), there are
 * S = ceil(m / segment) of them (the last may be short), and out192 receives S x 192 bytes, A_s || B_s.  A_s || B_s is byte for
 * byte what bp_verify_reduce returns for that slice of the proofs, public-input rows, weights and challenges alone: segment == 1
 * gives one pair per proof, segment >= m the one pair of bp_verify_reduce.  With segment == 1 a failing batch is located in ONE
 * call: the host sums the leaves of a range (bp_g1_bytes96_to_partial, bp_g1_sum_partials) and bisects with its pairing check.
 * weights == NULL (rho_j = 1) is accepted only when segment == 1 or m <= 1 -- a sum over several proofs needs caller-drawn
 * weights -- else BP_ERR_INVALID_ARG, as is segment == 0.  Every other argument rule, check and error is bp_verify_reduce's; any
 * rejection rejects the whole call and leaves out192 untouched.  m == 0: BP_OK, nothing written.  The work is 11 m + 9 S
 * variable-base multiplications, one per GPU lane, then short sums (no bucket MSM: a 20-term sum has no use for one).  Blocking;
 * ordered on the context's stream; a bp_init_multi context runs on its primary device. */
int  bp_verify_reduce_segments(bp_ctx* ctx, uint32_t log_n, const uint8_t vk768[768], const uint8_t* proofs624, size_t m,
                               const void* public_inputs, size_t n_public, const void* weights, const void* challenges,
                               int scalar_fmt, size_t segment, uint8_t* out192, size_t* first_bad);
/* HIP-event milliseconds of the stages of the last bp_verify_reduce or bp_verify_reduce_segments: upload, transcript, scalars,
 * decode + subgroup check, and the MSMs -- after bp_verify_reduce_segments: its multiplications, sums and encoding -- (all 0 after an
 * empty or a rejected batch). */
int  bp_verify_last_stats(bp_ctx* ctx, float stage_ms[5]);
/* The last stage of the last bp_verify_reduce_segments split in three: the multiplications; the per-proof sums, the segment tree and
 * the shared bases; normalisation and encoding. */
int  bp_verify_segments_last_stats(bp_ctx* ctx, float split_ms[3]);

/* ---- pairing checks: from the pairs of bp_verify_reduce(_segments) to verdicts (verifier.rs:187-191) ----
 * A G2 point is 192 bytes, G2Affine::to_uncompressed (g2.rs:284-303): x.c1 | x.c0 | y.c1 | y.c0, 48 big-endian bytes each, the flag
 * bits of the G1 encoding in the top of byte 0 (the identity is 0x40 and zeros).  A Gt element is 576 bytes, the memory image of Gt:
 * twelve Fp of six little-endian u64 Montgomery limbs, in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 -- so that two
 * implementations can be compared exactly, as with the 144-byte G1Projective image.
 *
 * The three calls below are host code and take no context (like bp_plonk_challenges). */
/* x_2 = k * G2 (setup.rs:20) for a canonical little-endian k; k >= q: BP_ERR_BAD_SCALAR; k = 0 gives the identity encoding. */
int  bp_g2_mul_generator(const uint8_t k32[32], uint8_t out192[192]);
/* bls12_381::pairing(p, q) of a G1 point (96 bytes) and a G2 point (192 bytes), both checked for canonical coordinates, flags and
 * the curve (not the subgroup): BP_ERR_BAD_POINT otherwise.  An identity on either side gives one. */
int  bp_pairing_gt_host(const uint8_t p96[96], const uint8_t q192[192], uint8_t gt576[576]);
/* n pairing checks against one setup.  pairs192 is n records A | B of 96 bytes each, exactly what bp_verify_reduce(_segments)
 * writes; verdicts[i] = 1 iff MillerLoop((A_i, x_2), (-B_i, G2)).final_exponentiation() == 1, i.e. pairing(A_i, x_2) ==
 * pairing(B_i, G2), else 0.  An identity G1 point drops its term, as multi_miller_loop does (pairings.rs:554-606): (identity,
 * identity) -- the pair of a weight-0 segment -- gives 1; (identity, B != 0) and (A != 0, identity) give 0.  gt576_or_null, when
 * not NULL, receives n x 576 bytes: the product after the final exponentiation.
 * Checks: every G1 point for canonical coordinates, flags and the curve; `checks & 1` adds the G1 subgroup test (not needed for
 * pairs of our own reduction), `checks & 2` the G2 subgroup test of x_2, which is always decoded and curve-checked.  A rejected G1
 * point is BP_ERR_BAD_POINT with the LOWEST failing pair index in *first_bad; a rejected x_2 is BP_ERR_BAD_POINT with *first_bad =
 * SIZE_MAX; an identity x_2 (tau = 0 is not a setup) and a NULL pointer are BP_ERR_INVALID_ARG.  Any rejection leaves verdicts and
 * gt untouched.  On success *first_bad = SIZE_MAX.  n == 0: BP_OK, verdicts and gt not written (and may be NULL). */
int  bp_pairing_check_host(const uint8_t x2_192[192], const uint8_t* pairs192, size_t n, uint32_t checks,
                           uint8_t* verdicts, uint8_t* gt576_or_null, size_t* first_bad);
/* The same on the GPU, one check per lane: same arguments, same rules, same bytes.  All G2 work (x_2's checks, the prepared lines
 * of x_2 and of the generator) is host work done once per call.  Blocking; ordered on the context's stream; a bp_init_multi
 * context runs on its primary device; buffers are workspaces of the context (a second call of the same size allocates nothing). */
int  bp_pairing_check(bp_ctx* ctx, const uint8_t x2_192[192], const uint8_t* pairs192, size_t n, uint32_t checks,
                      uint8_t* verdicts, uint8_t* gt576_or_null, size_t* first_bad);
/* Milliseconds of the stages of the last bp_pairing_check: preparing the lines, upload and decoding; the Miller loops; the final
 * exponentiations (all 0 after an empty call). */
int  bp_pairing_last_stats(bp_ctx* ctx, float stage_ms[3]);

/* ---- KZG openings in the basis of the SRS, and their batch check ----
 * bp_kzg_open_device opens `count` polynomials f_0 .. f_{count-1} at ONE point z: y_out receives the count values f_j(z) (32 bytes
 * each) and w96 the proof W = [q(tau)] G for q = (g - g(z)) / (x - z), g = sum_j nu^j f_j -- one proof for all of them.  The
 * polynomials stay in the form they are held in: against a Lagrange SRS (bp_srs_lagrange) the values come from the barycentric
 * formula, the quotient is a pointwise expression over one batched inversion (z on the domain included: the value is then
 * f_{j,m} and q_m the closed form of the derivative), and the proof is one commit to the same SRS -- no transform anywhere.
 * Against a powers-of-tau SRS the quotient is the TRUE quotient (max_j n_j - 1 coefficients; unlike bp_poly_div nothing is squeezed
 * out).
 *   d_polys, n     count pointers to HBM-resident Montgomery vectors on the context's primary device, and their lengths; n_j = 0 is
 *                  the zero polynomial (its pointer is ignored).  1 <= count <= 16, else BP_ERR_INVALID_ARG.
 *   basis          must be the basis of the SRS (bp_srs_basis), else BP_ERR_BASIS.  BP_BASIS_LAGRANGE: every n_j == srs_len, else
 *                  BP_ERR_LENGTH.  BP_BASIS_MONOMIAL: max_j n_j - 1 <= srs_len, else BP_ERR_LENGTH (a commit would silently stop
 *                  at the end of the SRS, and the proof would be false).
 *   z32, nu32      the point and the combiner, in scalar_fmt; nu32 may be NULL only with count == 1 (BP_ERR_INVALID_ARG otherwise).
 *                  y_out is written in scalar_fmt too.  A canonical-bytes scalar >= q is BP_ERR_BAD_SCALAR.
 * An empty or zero quotient gives the identity encoding, 0x40 then zeros.  An unknown handle is BP_ERR_INVALID_ARG.  A
 * bp_init_multi context does the field work on its primary device and the commit through its sharded SRS.  Blocking. */
int  bp_kzg_open_device(bp_ctx* ctx, uint64_t srs_handle, const void* const* d_polys, const size_t* n, size_t count, int basis,
                        const void* z32, const void* nu32_or_null, int scalar_fmt, void* y_out, uint8_t w96[96]);
/* The same for polynomials in host memory, in scalar_fmt (a BP_FR_BYTES_LE value >= q is BP_ERR_BAD_SCALAR). */
int  bp_kzg_open(bp_ctx* ctx, uint64_t srs_handle, const void* const* polys, const size_t* n, size_t count, int basis,
                 const void* z32, const void* nu32_or_null, int scalar_fmt, void* y_out, uint8_t w96[96]);
/* m claims "the commitments C_{i,0} .. C_{i,count-1} open at z_i to y_{i,0} .. y_{i,count-1}, combined by nu_i, with proof W_i"
 * reduced to two G1 points: out192 = A || B in the record format of bp_pairing_check, with
 *   A = sum_i r_i W_i
 *   B = sum_i r_i (sum_j nu_i^j (C_ij - y_ij G) + z_i W_i)
 * The batch holds iff pairing(A, x_2) == pairing(B, G2Affine::generator()) (up to the 2^-128 of the weights); this call does not
 * decide it.
 *   commitments96  m x count records, row i = claim i;  proofs96: m records;  z, nu, weights: m scalars;  y: m x count scalars, all
 *                  in scalar_fmt (a canonical-bytes value >= q: BP_ERR_BAD_SCALAR with the lowest such claim in *first_bad).
 *   nu_or_null     NULL only with count == 1.  1 <= count <= 16.
 *   weights        m scalars r_i, drawn by the caller AFTER it has received the claims, 128 bits of entropy or more each.  NULL means
 *                  r_i = 1 and is accepted for m <= 1 only (BP_ERR_INVALID_ARG otherwise).
 *   checks         every point is always checked for canonical coordinates, flags and the curve; checks & 1 adds the subgroup test.
 *                  A rejected point is BP_ERR_BAD_POINT with the lowest failing claim in *first_bad (may be NULL); out192 is then left
 *                  untouched.  On success *first_bad = SIZE_MAX.
 * m == 0: BP_OK, A = B = identity.  The scalars are computed on the host, the points decoded and summed (two MSMs over
 * m count + m + 1 and m points) on the context's primary device.  Blocking. */
int  bp_kzg_verify_reduce(bp_ctx* ctx, const uint8_t* commitments96, size_t m, size_t count, const void* z, const void* y,
                          const void* nu_or_null, const uint8_t* proofs96, const void* weights_or_null, int scalar_fmt,
                          uint32_t checks, uint8_t out192[192], size_t* first_bad);
/* Milliseconds of the last opening's two stages -- values and quotient; the commit -- and of the last bp_kzg_verify_reduce. */
int  bp_kzg_last_stats(bp_ctx* ctx, float ms[3]);

/* ---- all n = 2^log_n opening proofs of ONE polynomial on its domain (Feist, Khovratovich) ----
 * Proof i opens f at w^i, w = root_of_unity(n): pi_i = [(f(tau) - f(w^i)) / (tau - w^i)] G.  The n quotient commitments are one
 * Toeplitz product of the coefficients with the first n - 1 SRS points (a cyclic convolution of length 2n: one Fr transform, one
 * transform over G1 whose first pass multiplies entry j of a prepared table by its own scalar) followed by one DFT of length n over
 * G1: O(n log n) group operations instead of the n MSMs of n calls of bp_kzg_open.
 *   srs_handle   a powers-of-tau SRS (BP_BASIS_MONOMIAL; a Lagrange handle is BP_ERR_BASIS).  Only its first n - 1 points are used;
 *                n - 1 > srs_len is BP_ERR_LENGTH.  An unknown handle is BP_ERR_INVALID_ARG.
 *   log_n        log_n >= 24 is BP_ERR_TOO_LARGE (the transform of 2n points is the limit).  log_n == 0: one proof, the identity, and
 *                the value f_0; no kernel runs.
 *   poly, basis  BP_BASIS_MONOMIAL: n_values <= n coefficients (more: BP_ERR_LENGTH; fewer: zero-padded; 0: the zero polynomial, poly
 *                may then be NULL).  BP_BASIS_LAGRANGE: exactly n values f(w^i) (BP_ERR_LENGTH otherwise), transformed internally by
 *                one inverse NTT; the returned values are then the input itself.
 *   values       n scalars f(w^i) in scalar_fmt, or NULL.   proofs96: n x 96 bytes, natural order (identity = 0x40, zeros).
 * A BP_FR_BYTES_LE input >= q is BP_ERR_BAD_SCALAR.  Null pointers and a bad format or basis are BP_ERR_INVALID_ARG.  A rejected call
 * writes nothing.  Blocking, ordered on the context's stream.  A bp_init_multi context collects the points on its primary device (as
 * bp_srs_lagrange does) and runs there.
 *
 * bp_srs_open_all_prepare builds and keeps the table DFT_2n(S^) for this SRS and log_n (2n x 96 bytes of HBM, released by
 * bp_srs_free; a later call with another log_n replaces it).  Optional: bp_kzg_open_all builds it on first use. */
int  bp_srs_open_all_prepare(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n);
int  bp_kzg_open_all(bp_ctx* ctx, uint64_t srs_handle, const void* poly, size_t n_values, int basis, int scalar_fmt,
                     uint32_t log_n, void* values, uint8_t* proofs96);
/* The same for a polynomial resident in HBM on the context's primary device (Montgomery); values_mont_host: n Montgomery scalars in
 * HOST memory, or NULL. */
int  bp_kzg_open_all_device(bp_ctx* ctx, uint64_t srs_handle, const void* d_poly, size_t n_values, int basis,
                            uint32_t log_n, void* values_mont_host, uint8_t* proofs96);
/* HIP-event ms of the last bp_kzg_open_all(_device): table build (0 when it was already there), field work (with the twiddle tables
 * of the G1 transforms when the table was there but the context has no twiddles for this log_n; a table build makes them itself),
 * Toeplitz transform, final transform + normalisation + encoding. */
int  bp_kzg_open_all_last_stats(bp_ctx* ctx, float stage_ms[4]);

/* ---- cell proofs: the n / l coset multi-proofs of ONE polynomial in one call, and the reduction of m cell claims ----
 * n = 2^log_n, l = 2^log_l <= n, r = n / l, w = root_of_unity(n).  Cell k < r is the coset { w^(k + r j) : j < l }; its values are
 * v_{k,j} = f(w^(k + r j)) and its ONE proof is pi_k = [q_k(tau)] G with q_k = f div (x^l - a_k), a_k = w^(k l): the second half of
 * Feist, Khovratovich, and the shape of a data-availability cell.  l Toeplitz products of length r are summed (a table of l
 * transforms of 2r points side by side, ONE batched Fr transform, two scalar multiplications per GPU lane and log_l - 1 passes of
 * additions), one inverse transform of 2r points and one DFT of r points over G1 follow.  log_l = 0 is bp_kzg_open_all, byte for byte.
 *   srs_handle, poly, basis, scalar_fmt: as for bp_kzg_open_all.  Only the first n - l points are used; n - l > srs_len is BP_ERR_LENGTH.
 *   log_n, log_l   log_l > log_n is BP_ERR_INVALID_ARG, log_n >= 24 BP_ERR_TOO_LARGE.  log_l == log_n: one proof, the identity (the
 *                  quotient is zero); the values are written and no kernel over G1 runs.
 *   values         n scalars in CELL ORDER, values[k l + j] = f(w^(k + r j)), or NULL.   proofs96: r x 96 bytes, proof k of cell k.
 * A rejected call writes nothing.  Stage times: bp_kzg_open_all_last_stats (table | field work | multiplication, halving and inverse
 * transform | final transform, normalisation, encoding).  A bp_init_multi context collects the points on its primary device.
 *
 * bp_srs_open_cosets_prepare builds and keeps the table for (log_n, log_l): 2n x 96 bytes, in the SRS's ONE table slot.  The slot's
 * key is (log_n, log_l) and bp_srs_open_all_prepare / bp_kzg_open_all use log_l = 0: a call with another key replaces the table. */
int  bp_srs_open_cosets_prepare(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint32_t log_l);
int  bp_kzg_open_cosets(bp_ctx* ctx, uint64_t srs_handle, const void* poly, size_t n_values, int basis, int scalar_fmt,
                        uint32_t log_n, uint32_t log_l, void* values, uint8_t* proofs96);
int  bp_kzg_open_cosets_device(bp_ctx* ctx, uint64_t srs_handle, const void* d_poly, size_t n_values, int basis,
                               uint32_t log_n, uint32_t log_l, void* values_mont_host, uint8_t* proofs96);
/* m cell claims (C_i, k_i, v_{i,0} .. v_{i,l-1}, pi_i) reduced to out192 = A || B, the record of bp_pairing_check:
 *   A = sum_i rho_i pi_i          B = sum_i rho_i (C_i + a_{k_i} pi_i) - sum_{t<l} (sum_i rho_i c_{i,t}) P_t
 * with c_{i,t} = w^(-k_i t) l^-1 sum_j v_{i,j} zeta^(-j t), zeta = w^r: the coefficients of the interpolant of the values on the coset.
 * The batch holds iff pairing(A, [tau^l]_2) == pairing(B, G2Affine::generator()): bp_pairing_check with [tau^l]_2 passed where x_2
 * goes.  That G2 point is the CALLER'S (ceremonies ship the G2 powers); this call does not decide the pairing.
 *   srs_handle   a powers-of-tau SRS with at least l points (BP_ERR_BASIS, BP_ERR_LENGTH).  log_l > log_n: BP_ERR_INVALID_ARG; log_n >= 24: BP_ERR_TOO_LARGE.
 *   cell_index   m indices; one >= r is BP_ERR_INVALID_ARG with the claim in *first_bad.
 *   values       m x l scalars in scalar_fmt, row i = claim i in the cell order of bp_kzg_open_cosets; a canonical-bytes value >= q
 *                (or weight) is BP_ERR_BAD_SCALAR with the claim in *first_bad.
 *   weights, checks, first_bad, m == 0: as for bp_kzg_verify_reduce.
 * One batched inverse Fr transform of the m rows, one kernel for the weights and sums, two MSMs (over 2m + l and m points).  Blocking. */
int  bp_kzg_verify_cells_reduce(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint32_t log_l, const uint8_t* commitments96,
                                const uint32_t* cell_index, const void* values, const uint8_t* proofs96, size_t m,
                                const void* weights_or_null, int scalar_fmt, uint32_t checks, uint8_t out192[192], size_t* first_bad);

/* ---- cell recovery: ONE polynomial, all its r cells and all r proofs rebuilt from m of the cells ----
 * The third operation of a data-availability scheme (PeerDAS: recover_cells_and_kzg_proofs).  n, l, r, w and the cells as above;
 * w_r = w^l.  Given m distinct cell indices in any order, their m x l values (row i = the cell cell_index[i], in cell order) and a
 * degree bound n_coeffs = d (deg f < d, 1 <= d <= m l), with M the r - m missing indices and Z(x) = prod_{k in M} (x^l - w_r^k):
 * Z is evaluated on the domain and on the domain shifted by s = 7 directly, r values each (its coefficients are never formed);
 * (f Z) on the domain is the given values times Z, zero on the missing cells; one inverse transform, then a forward transform on the
 * shifted domain, the division by Z there and one more inverse transform give g, the interpolant of the given values (deg g < m l).
 * Four Fr transforms of length n (one when nothing is missing) and 2 r |M| products; nothing over G1.
 *   cell_index    host memory, m indices.  One >= r is BP_ERR_INVALID_ARG with its position in *first_bad; a repeated one
 *                 BP_ERR_INVALID_ARG with the position of the second occurrence.  These come first, then:
 *   n_coeffs      0, > n or > m l (too few cells) is BP_ERR_LENGTH.
 *   log_n, log_l  log_l > log_n is BP_ERR_INVALID_ARG; log_n >= 24 or r > 2^16 is BP_ERR_TOO_LARGE (Z is evaluated directly: at most
 *                 2^33 products under this limit).  In a shape that is refused a repeated index is not looked for.
 *   values        a canonical-bytes value >= q is BP_ERR_BAD_SCALAR with the cell's position in *first_bad.
 *   consistency   the cells agree with SOME polynomial of degree < d exactly when coefficients d .. n - 1 of g are zero; otherwise
 *                 the call fails with BP_ERR_ASSERT and *first_bad = the lowest non-zero coefficient index (it does not say which cell
 *                 is wrong).  With m l == d there is no redundancy and NOTHING to check: the call returns the interpolant of
 *                 whatever it was given, and a wrong value goes unnoticed.
 *   first_bad     may be NULL; SIZE_MAX when no position applies.
 * bp_kzg_recover: values and coeffs_out (n_coeffs scalars) in host memory, in scalar_fmt.
 * bp_kzg_recover_device: d_values (m l Montgomery elements) and d_coeffs (room for n Montgomery elements, apart from d_values) in HBM
 * on the context's primary device; the work is done in d_coeffs: on BP_OK its first n_coeffs elements are the result and the rest zero,
 * after BP_ERR_ASSERT it holds the n coefficients of the interpolant (unspecified for callers), after any other refusal it is untouched.
 * bp_kzg_recover_cells: the recovery, then the core of bp_kzg_open_cosets_device on the coefficients where they lie (they never
 * leave HBM): values_out (n scalars in scalar_fmt, cell order, or NULL) and proofs96 (r x 96 bytes) are ALL cells and proofs, the
 * given ones included.  SRS requirements and errors are bp_kzg_open_cosets' (a powers-of-tau SRS, n - l <= srs_len), checked after
 * the rules above and before anything is computed; the proof stages' times stay in bp_kzg_open_all_last_stats.
 * A rejected call writes nothing to its host outputs.  Null context or pointers and a bad format are BP_ERR_INVALID_ARG.  A
 * bp_init_multi context runs on its primary device.  Blocking; ordered on the context's stream.
 * bp_kzg_recover_last_stats: HIP-event milliseconds of the last accepted recovery: vanishing evaluations | spread + first inverse
 * transform | coset division (three transforms) | check + output.  Entries 0 and 2 are 0 when no cell was missing; all four are 0
 * after a call that BP_ERR_ASSERT refused. */
int  bp_kzg_recover(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const void* values, size_t m,
                    size_t n_coeffs, int scalar_fmt, void* coeffs_out, size_t* first_bad);
int  bp_kzg_recover_device(bp_ctx* ctx, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index, const void* d_values, size_t m,
                           size_t n_coeffs, void* d_coeffs, size_t* first_bad);
int  bp_kzg_recover_cells(bp_ctx* ctx, uint64_t srs_handle, uint32_t log_n, uint32_t log_l, const uint32_t* cell_index,
                          const void* values, size_t m, size_t n_coeffs, int scalar_fmt, void* values_out, uint8_t* proofs96,
                          size_t* first_bad);
int  bp_kzg_recover_last_stats(bp_ctx* ctx, float stage_ms[4]);

/* ---- the structure of an SRS: powers of one tau, Lagrange points that belong to them, a ceremony contribution ----
 * bp_srs_load* and bp_srs_check_subgroup say that every point is a point of G1; nothing there says that the points are
 * G, tau G, tau^2 G, ... for ONE tau, or that x_2 is that tau in G2.  The calls below do, without knowing tau.
 *
 * bp_srs_powers_reduce: out192 = A || B (the record of bp_pairing_check) with
 *   A = sum_{i < n_pairs} rho^i P_{first+i}        B = sum_{i < n_pairs} rho^i P_{first+i+1}
 * Every pair satisfies P_{i+1} = tau P_i exactly when pairing(A, x_2) == pairing(B, G2Affine::generator()); if one pair does not,
 * a rho drawn AFTER the points were fixed, with 128 bits of entropy or more, hides it with probability at most n_pairs / 2^127.  The
 * two pairings stay with the caller, as with bp_verify_reduce.  Two MSMs (at `first` and `first + 1`, through the SRS's tables where
 * it has them, over every shard of a bp_init_multi context) against ONE vector rho^i made on the device.
 *   first + n_pairs + 1 > srs_len: BP_ERR_INVALID_ARG.  n_pairs == 0: BP_OK, A = B = identity.  A Lagrange SRS: BP_ERR_BASIS.
 *   rho32 in scalar_fmt: a canonical-bytes value >= q is BP_ERR_BAD_SCALAR; rho < 2 is BP_ERR_INVALID_ARG (rho = 1 lets errors cancel,
 *   rho = 0 looks at one pair). */
int  bp_srs_powers_reduce(bp_ctx* ctx, uint64_t srs_handle, size_t first, size_t n_pairs, const void* rho32, int scalar_fmt,
                          uint8_t out192[192]);
/* The verdict: one reduce over all srs_len - 1 pairs and one pairing check on the host (the code of bp_pairing_check_host; x_2 is
 * decoded, curve- and subgroup-checked: a rejected x_2 is BP_ERR_BAD_POINT with *first_bad = SIZE_MAX, an identity x_2
 * BP_ERR_INVALID_ARG).  BP_OK with *first_bad = SIZE_MAX: the points are the powers of the tau of x_2 (up to (srs_len - 1) / 2^127).
 * BP_ERR_BAD_POINT otherwise, with *first_bad = the lowest i >= 1 such that P_i != tau P_{i-1} relative to x_2 (bp_last_error names
 * it), found by bisection over the prefixes [0, k) of the pairs against the rho^i already on the device: a call makes at most
 * 2 + ceil(log2(srs_len)) reduces and as many pairings, whatever it finds (bp_srs_check_last_stats).  A wrong x_2 fails every pair:
 * *first_bad = 1.  checks & BP_SRS_CHECK_GENERATOR: P_0 must be G1Affine::generator() (a ceremony's first point; compared first, on
 * the host): else *first_bad = 0.  Any other bit of checks is BP_ERR_INVALID_ARG.  srs_len <= 1 has no pair: BP_OK.  rho32 and the
 * basis rule as bp_srs_powers_reduce.  first_bad may be NULL.  Blocking. */
#define BP_SRS_CHECK_GENERATOR 2u
int  bp_srs_check_powers(bp_ctx* ctx, uint64_t srs_handle, const uint8_t x2_192[192], const void* rho32, int scalar_fmt,
                         uint32_t checks, size_t* first_bad);
/* reduces (for bp_srs_adopt_lagrange: comparisons of two MSMs), host pairings and host wall-clock milliseconds of the last
 * bp_srs_check_powers or bp_srs_adopt_lagrange on this ctx.  Any pointer may be null. */
int  bp_srs_check_last_stats(bp_ctx* ctx, uint32_t* reduces, uint32_t* pairings, float* ms);
/* A Lagrange-basis SRS that was SHIPPED (the Ethereum KZG ceremony's G1 points; an exported bp_srs_lagrange) instead of computed:
 * `points` is a Monomial-tagged handle of exactly 2^log_n points from any loader (another length: BP_ERR_LENGTH), `powers` a
 * Monomial handle of at least 2^log_n points (fewer: BP_ERR_INVALID_ARG) that bp_srs_check_powers has accepted.  With v_i = rho^i and
 * c = i_ntt_381(v), the points are the Lagrange points of the powers exactly when sum_i v_i points_i == sum_j c_j powers_j as group
 * elements (both sides commit to the polynomial with values v): two MSMs and one transform, no pairing, no x_2, error probability
 * at most 2^log_n / 2^127 for a rho drawn after the points were fixed.  On success *lagrange_handle is a NEW handle -- a device-to-
 * device copy of the points tagged BP_BASIS_LAGRANGE with this log_n, in every respect what bp_srs_lagrange returns -- and both
 * sources are untouched.  On failure BP_ERR_BAD_POINT, no handle, and *first_bad (may be NULL) = the lowest wrong index, found by
 * the bisection of bp_srs_check_powers with v zeroed from k on (one transform and two MSMs per step, the same bound on the steps).
 * A Lagrange handle on either side: BP_ERR_BASIS.  log_n > 24: BP_ERR_TOO_LARGE.  rho32 as bp_srs_powers_reduce.  Blocking. */
int  bp_srs_adopt_lagrange(bp_ctx* ctx, uint64_t points_handle, uint64_t powers_handle, uint32_t log_n, const void* rho32,
                           int scalar_fmt, uint64_t* lagrange_handle, size_t* first_bad);
/* out_i = k_i * P_i for all n == srs_len points (another n: BP_ERR_LENGTH) as a new SRS of the same basis and log_n: one variable-
 * base multiplication per GPU lane.  With k_i = s^i this is a contribution to a ceremony, P_i <- s^i P_i (x_2 <- s x_2: bp_g2_mul).
 * The source is ALWAYS subgroup-tested first (the test of bp_srs_check_subgroup): the multiplication is the 128-step split form,
 * exact only inside the prime-order subgroup, and a contribution to points outside it means nothing -- a point outside is
 * BP_ERR_BAD_POINT with its index in *first_bad (may be NULL; SIZE_MAX otherwise) and no handle.  An identity point stays the
 * identity; k_i = 0 gives the identity.  scalars: n values in scalar_fmt, in host memory or (scalars_on_device != 0) in HBM of the
 * primary device; a canonical-bytes value >= q is BP_ERR_BAD_SCALAR, no handle.  On a bp_init_multi context every shard scales its
 * own range with its slice of the scalars, and the result is sharded like the source.  Blocking. */
int  bp_srs_scale(bp_ctx* ctx, uint64_t srs_handle, const void* scalars, size_t n, int scalar_fmt, int scalars_on_device,
                  uint64_t* out_handle, size_t* first_bad);
/* HIP-event milliseconds of the last bp_srs_scale on this ctx: the subgroup test, the multiplications (srs_scale), the normalisation;
 * summed over the shards of a bp_init_multi context (all 0 after a call refused for its length). */
int  bp_srs_scale_last_stats(bp_ctx* ctx, float stage_ms[3]);
/* Host-side, no context: out = k * Q in G2 for a canonical little-endian k (k >= q: BP_ERR_BAD_SCALAR).  Q is decoded and curve-
 * checked (BP_ERR_BAD_POINT), not subgroup-checked; an identity Q or k = 0 gives the identity encoding. */
int  bp_g2_mul(const uint8_t q192[192], const uint8_t k32[32], uint8_t out192[192]);

#ifdef __cplusplus
}
#endif
#endif
