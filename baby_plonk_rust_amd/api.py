"""Host-side mirror of the reference's interface for the hot path, on top of the C ABI.

Names, argument meaning and error behaviour follow the reference (Rust) so the parity tests read like its
own tests; where the reference panics (assert!/unwrap) these raise BpError/AssertionError.

  reference (file:line)                               here
  ---------------------------------------------------------------------------------------------
  Setup::generate_srs(powers, tau)   setup.rs:12-31   Setup.generate_srs(powers, tau)
  Setup::commit(&poly)               setup.rs:32-37   Setup.commit(poly)
  (no counterpart: KZG open / check)                  Setup.open(polys, z, nu) / Setup.verify_openings(openings)
  (no counterpart: ceremony files)                    Setup.check_powers() / from_lagrange_points() / contribute(s) / verify_contribution()
  BucketMSM::bucket_msm(p, s, b, c)  msm.rs:76-118    BucketMSM.bucket_msm(points, scalars, b, c)
  ntt_381 / i_ntt_381                utils.rs:63,106  ntt_381(values) / i_ntt_381(values)
  root_of_unity / roots_of_unity     utils.rs:39-52   root_of_unity(n) / roots_of_unity(n)
  Polynomial{values,basis} + ops     polynomial.rs    Polynomial(values, basis) with + - * / and methods

Scalars travel as numpy uint64 arrays of shape [n, 4]: the reference's Montgomery limbs (Scalar::to_array,
scalar.rs:35-40).  Points travel in the 96-byte uncompressed encoding (g1.rs:246-260)."""
import collections
import ctypes as C

import os

import numpy as np

from . import _lib
from ._lib import BASIS_LAGRANGE, BASIS_MONOMIAL, FR_BYTES_LE, FR_MONT, BpError

SRS_TABLES_OFF = 1      # bp_srs_precompute(window_bits): drop the fixed-base tables

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
_R = pow(2, 256, Q)
_RINV = pow(_R, Q - 2, Q)


def scalar_from_int(v):
    """Scalar::from / from_raw: canonical integer -> Montgomery limbs (host-side big-int, O(1))"""
    m = (v % Q) * _R % Q
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def scalar_to_int(limbs):
    m = sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(limbs, dtype=np.uint64).reshape(4)))
    return m * _RINV % Q


def scalars_from_ints(vals):
    return np.stack([scalar_from_int(v) for v in vals]) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def scalars_to_ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [scalar_to_int(a[i]) for i in range(len(a))]


def _fr_array(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim == 1:
        a = a.reshape(-1, 4)
    assert a.ndim == 2 and a.shape[1] == 4, a.shape
    return a


_SIZE_MAX = C.c_size_t(-1).value


def _scalar32(v):
    """an integer as the 32 little-endian bytes of BP_FR_BYTES_LE, NOT reduced: the library refuses a value >= q"""
    if not 0 <= int(v) < 1 << 256:
        raise BpError(-4, "scalar", "outside 0 .. 2^256")
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8).copy()


def _draw_rho():
    """128 random bits with the top bit set: the weight of a random linear combination, drawn once the data is in hand"""
    import secrets
    return secrets.randbits(128) | 1 << 127


class Context:
    """bp_ctx: one GPU (device = int, bp_init) or one context over several GPUs (device = list of ids, bp_init_multi:
    SRS and MSMs sharded by point range inside the library, everything else on the first device).
    The module keeps a default context per device."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (C.c_int * len(device))(*device)
            rc = self._lib.bp_init_multi(C.byref(h), ids, len(device))
            self.devices = list(device)
        else:
            rc = self._lib.bp_init(C.byref(h), device)
            self.devices = [device]
        if rc != 0:
            raise BpError(rc, "bp_init", "no usable GPU: this package has no CPU fallback")
        self._h = h
        self.device = self.devices[0]
        self._async_keepalive = []       # host buffers handed to *_async calls: referenced until the next synchronize()

    def n_shards(self):
        return self._lib.bp_ctx_devices(self._h, None, 0)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, where):
        if rc != 0:
            raise BpError(rc, where, (self._lib.bp_last_error(self._h) or b"").decode())

    # ---- thin wrappers -----------------------------------------------------------------------
    def srs_load(self, points96):
        buf = np.ascontiguousarray(np.frombuffer(bytes(points96), dtype=np.uint8))
        n, h = len(buf) // 96, C.c_uint64()
        self.check(self._lib.bp_srs_load(self._h, buf.ctypes.data, n, C.byref(h)), "bp_srs_load")
        return h.value

    def srs_load_projective144(self, points144):
        """n x 144 bytes: the in-memory image of G1Projective (x | y | z Montgomery limbs), normalised on the GPU"""
        buf = points144 if isinstance(points144, np.ndarray) else np.frombuffer(bytes(points144), dtype=np.uint8)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        n, h = len(buf) // 144, C.c_uint64()
        self.check(self._lib.bp_srs_load_projective144(self._h, buf.ctypes.data, n, C.byref(h)), "bp_srs_load_projective144")
        return h.value

    def srs_load_compressed48(self, points48, check_subgroup=True):
        """n x 48 bytes in the compressed encoding (a ceremony file's records as they are), decoded on the GPU:
        G1Affine::from_compressed, or from_compressed_unchecked with check_subgroup=False.  A rejected point raises
        BpError(BP_ERR_BAD_POINT) whose text names the lowest failing index (also in the exception's `index`)"""
        buf = points48 if isinstance(points48, np.ndarray) else np.frombuffer(bytes(points48), dtype=np.uint8)
        buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
        n, h, bad = len(buf) // 48, C.c_uint64(), C.c_size_t()
        rc = self._lib.bp_srs_load_compressed48(self._h, buf.ctypes.data, n, _lib.SRS_CHECK_SUBGROUP if check_subgroup else 0, C.byref(h),
                                                C.byref(bad))
        try:
            self.check(rc, "bp_srs_load_compressed48")
        except BpError as e:
            e.index = bad.value if rc == -3 else None
            raise
        return h.value

    def srs_export_compressed48(self, handle, first=0, n=None):
        """points [first, first + n) in the 48-byte compressed encoding (G1Affine::to_compressed), encoded on the GPU"""
        n = self.srs_len(handle) - first if n is None else n
        out = np.zeros(48 * n, dtype=np.uint8)
        self.check(self._lib.bp_srs_export_compressed48(self._h, handle, first, n, out.ctypes.data), "bp_srs_export_compressed48")
        return bytes(out)

    def srs_check_subgroup(self, handle, first=0, n=None):
        """is_torsion_free over points [first, first + n) of any SRS, on the GPU: None, or the lowest index outside the subgroup"""
        n = self.srs_len(handle) - first if n is None else n
        bad = C.c_size_t()
        rc = self._lib.bp_srs_check_subgroup(self._h, handle, first, n, C.byref(bad))
        if rc == -3:
            return bad.value
        self.check(rc, "bp_srs_check_subgroup")
        return None

    def msm_projective144(self, points144, scalars, fmt=FR_MONT):
        """BucketMSM::bucket_msm(&[G1Projective], &[Scalar]) in one call, nothing cached: upload in two pieces, multiply the first behind the upload of the second"""
        buf = points144 if isinstance(points144, np.ndarray) else np.frombuffer(bytes(points144), dtype=np.uint8)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        s = _fr_array(scalars) if fmt == FR_MONT else np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros(96, dtype=np.uint8)
        self.check(self._lib.bp_msm_g1_projective144(self._h, buf.ctypes.data, len(buf) // 144, s.ctypes.data, len(s), fmt, out.ctypes.data),
                   "bp_msm_g1_projective144")
        return out.tobytes()

    def srs_generate(self, powers, tau_int):
        t, h = np.frombuffer((tau_int % Q).to_bytes(32, "little"), dtype=np.uint8).copy(), C.c_uint64()
        self.check(self._lib.bp_srs_generate(self._h, powers, t.ctypes.data, C.byref(h)), "bp_srs_generate")
        return h.value

    def srs_generate_progression(self, n, a_int, d_int):
        a = np.frombuffer((a_int % Q).to_bytes(32, "little"), dtype=np.uint8).copy()
        d = np.frombuffer((d_int % Q).to_bytes(32, "little"), dtype=np.uint8).copy()
        h = C.c_uint64()
        self.check(self._lib.bp_srs_generate_progression(self._h, n, a.ctypes.data, d.ctypes.data, C.byref(h)),
                   "bp_srs_generate_progression")
        return h.value

    def srs_len(self, handle):
        n = C.c_size_t()
        self.check(self._lib.bp_srs_len(self._h, handle, C.byref(n)), "bp_srs_len")
        return n.value

    def srs_export(self, handle, first=0, n=None):
        n = self.srs_len(handle) - first if n is None else n
        out = np.zeros(96 * n, dtype=np.uint8)
        self.check(self._lib.bp_srs_export(self._h, handle, first, n, out.ctypes.data), "bp_srs_export")
        return bytes(out)

    def srs_export_projective144(self, handle, first=0, n=None):
        """the points as G1Projective memory images (144 bytes each, z = 1): what a Rust Vec<G1Projective> holds"""
        n = self.srs_len(handle) - first if n is None else n
        out = np.zeros(144 * n, dtype=np.uint8)
        self.check(self._lib.bp_srs_export_projective144(self._h, handle, first, n, out.ctypes.data), "bp_srs_export_projective144")
        return out

    def srs_lagrange(self, handle, log_n):
        """the Lagrange-basis SRS [L_i(tau)] G over the 2^log_n-th roots of unity, from the first 2^log_n points of a powers-of-tau
        SRS: the inverse NTT taken in G1, on the GPU, tau unknown (bp_srs_lagrange).  Returns a new SRS handle; the source stays"""
        h = C.c_uint64()
        self.check(self._lib.bp_srs_lagrange(self._h, handle, log_n, C.byref(h)), "bp_srs_lagrange")
        return h.value

    def srs_basis(self, handle):
        """(BASIS_MONOMIAL, 0) for a loaded or generated SRS, (BASIS_LAGRANGE, log_n) for one made by srs_lagrange"""
        b, k = C.c_int(), C.c_uint32()
        self.check(self._lib.bp_srs_basis(self._h, handle, C.byref(b), C.byref(k)), "bp_srs_basis")
        return b.value, k.value

    def srs_free(self, handle):
        self.check(self._lib.bp_srs_free(self._h, handle), "bp_srs_free")

    def srs_precompute(self, handle, window_bits=0):
        """fixed-base window tables T[w][i] = 2^(c w) P_i for an SRS that serves many MSMs (0 = auto width,
        SRS_TABLES_OFF drops them, else 4..24; anything else raises BpError(BP_ERR_INVALID_ARG))"""
        self.check(self._lib.bp_srs_precompute(self._h, handle, window_bits), "bp_srs_precompute")
        return self.srs_table_info(handle)

    def srs_table_info(self, handle):
        c, w, b = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.check(self._lib.bp_srs_table_info(self._h, handle, C.byref(c), C.byref(w), C.byref(b)), "bp_srs_table_info")
        return {"window_bits": c.value, "windows": w.value, "bytes": b.value}

    def msm(self, handle, scalars, fmt=FR_MONT):
        s = _fr_array(scalars) if fmt == FR_MONT else np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros(96, dtype=np.uint8)
        self.check(self._lib.bp_msm_g1(self._h, handle, s.ctypes.data, len(s), fmt, out.ctypes.data), "bp_msm_g1")
        return bytes(out)

    def msm_partial(self, handle, scalars, first=0, fmt=FR_MONT, device_ptr=None, n=None):
        """144-byte projective partial over SRS[first:first+n]; scalars = host array or (device_ptr, n)"""
        out = np.zeros(144, dtype=np.uint8)
        if device_ptr is not None:
            rc = self._lib.bp_msm_g1_partial(self._h, handle, first, device_ptr, n, fmt, 1, out.ctypes.data)
        else:
            s = _fr_array(scalars)
            rc = self._lib.bp_msm_g1_partial(self._h, handle, first, s.ctypes.data, len(s), fmt, 0, out.ctypes.data)
        self.check(rc, "bp_msm_g1_partial")
        return bytes(out)

    def msm_blob_device(self, handle, d_blob_ptr, scalars=None, first=0, fmt=FR_MONT, device_ptr=None, n=None, wait=True):
        """one process per GPU: this rank's partial sums stay in HBM at d_blob_ptr (MSM_BLOB_BYTES), ready for the all-gather.
        wait=False: stream-ordered (bp_msm_g1_blob_device_async): enqueued on the context's stream (set_stream), not waited for"""
        fn = self._lib.bp_msm_g1_blob_device if wait else self._lib.bp_msm_g1_blob_device_async
        if device_ptr is not None:
            rc = fn(self._h, handle, first, device_ptr, n, fmt, 1, d_blob_ptr)
        else:
            s = _fr_array(scalars) if fmt == FR_MONT else np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
            if not wait:
                self._async_keepalive.append(s)      # the copy is stream-ordered (bp_msm_ntt.h): alive until synchronize()
            rc = fn(self._h, handle, first, s.ctypes.data, len(s), fmt, 0, d_blob_ptr)
        self.check(rc, "bp_msm_g1_blob_device" if wait else "bp_msm_g1_blob_device_async")

    def msm_blobs_sum_device(self, d_blobs_ptr, n_blobs, d_out_ptr, wait=True):
        """gathered records of equal layout -> one record, added slot by slot on the GPU (see bp_msm_blobs_sum_device)"""
        fn = self._lib.bp_msm_blobs_sum_device if wait else self._lib.bp_msm_blobs_sum_device_async
        self.check(fn(self._h, d_blobs_ptr, n_blobs, d_out_ptr), "bp_msm_blobs_sum_device")

    # ---- one process per GPU: the collective under the C ABI (capi_comm.hip) ----
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128-byte id every rank passes to comm_init_rank (ncclGetUniqueId); the host carries it between the ranks"""
        out = np.zeros(_lib.COMM_ID_BYTES, dtype=np.uint8)
        rc = _lib.load().bp_comm_unique_id(out.ctypes.data)
        if rc != 0:
            raise BpError(rc, "bp_comm_unique_id")
        return bytes(out)

    def comm_init_rank(self, comm_id, rank, world):
        buf = np.frombuffer(bytes(comm_id), dtype=np.uint8).copy()
        assert len(buf) == _lib.COMM_ID_BYTES
        self.check(self._lib.bp_comm_init_rank(self._h, buf.ctypes.data, rank, world), "bp_comm_init_rank")

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        self.check(self._lib.bp_comm_info(self._h, C.byref(r), C.byref(w)), "bp_comm_info")
        return r.value, w.value

    def comm_destroy(self):
        self.check(self._lib.bp_comm_destroy(self._h), "bp_comm_destroy")

    def comm_set_timeout_ms(self, ms):
        """bound of every wait behind a collective and of ncclCommInitRank (default 120 000 ms; 0 = none): when it expires the
        communicator is aborted and the call returns BP_ERR_COMM -- an error, not a stall"""
        self.check(self._lib.bp_comm_set_timeout_ms(self._h, int(ms)), "bp_comm_set_timeout_ms")

    def comm_stats(self):
        n, ms = C.c_uint64(), C.c_uint32()
        self.check(self._lib.bp_comm_stats(self._h, C.byref(n), C.byref(ms)), "bp_comm_stats")
        return {"collectives": n.value, "timeout_ms": ms.value}

    def msm_allgather(self, handle, scalars=None, first=0, fmt=FR_MONT, device_ptr=None, n=None):
        """sum over ALL ranks' (point, scalar) pairs (bp_msm_g1_allgather): record -> ONE ncclAllGather -> device pre-sum -> one D2H"""
        out = np.zeros(96, dtype=np.uint8)
        if device_ptr is not None:
            rc = self._lib.bp_msm_g1_allgather(self._h, handle, first, device_ptr, n, fmt, 1, out.ctypes.data)
        else:
            s = _fr_array(scalars) if fmt == FR_MONT else np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
            rc = self._lib.bp_msm_g1_allgather(self._h, handle, first, s.ctypes.data, len(s), fmt, 0, out.ctypes.data)
        self.check(rc, "bp_msm_g1_allgather")
        return bytes(out)

    def comm_last_exchange_ms(self):
        ms = C.c_float()
        self.check(self._lib.bp_comm_last_exchange_ms(self._h, C.byref(ms)), "bp_comm_last_exchange_ms")
        return ms.value

    def ntt_columns_allgather(self, d_columns_ptr, log_n, columns_per_rank):
        """world x columns_per_rank columns of 2^log_n elements in HBM, this rank's block filled: ONE in-place ncclAllGather"""
        self.check(self._lib.bp_ntt_columns_allgather(self._h, d_columns_ptr, log_n, columns_per_rank), "bp_ntt_columns_allgather")

    def msm_stats(self):
        a, t, adds, c = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint32()
        self.check(self._lib.bp_msm_last_stats(self._h, C.byref(a), C.byref(t), C.byref(adds), C.byref(c)), "bp_msm_last_stats")
        return {"accumulate_ms": a.value, "device_ms": t.value, "mixed_adds": adds.value, "window_bits": c.value,
                "tables": self._lib.bp_msm_last_used_tables(self._h) == 1}

    MSM_PATH_FIELDS = ("J", "c", "W", "radix", "sort", "pb", "packed", "flat", "wide8", "fixup", "n_wide", "chunk")

    def msm_path(self, member=0):
        """which path the last MSM pipeline on a member's context took (bp_msm_last_path): J vectors, c, W, radix, sort (1 two-level,
        2 partition), pb, packed, flat, wide8, fixup (0 per bucket, 1 per edge), n_wide, chunk"""
        out = (C.c_uint32 * 12)()
        self.check(self._lib.bp_msm_last_path(self._h, member, out), "bp_msm_last_path")
        return dict(zip(self.MSM_PATH_FIELDS, (int(v) for v in out)))

    def msm_member_stats(self):
        """per member of a group context: upload (host scalars only), accumulate and whole-pipeline device times of the last MSM"""
        out = []
        for r in range(self.n_shards()):
            u, a, t, adds = C.c_float(), C.c_float(), C.c_float(), C.c_uint64()
            self.check(self._lib.bp_msm_last_member_stats(self._h, r, C.byref(u), C.byref(a), C.byref(t), C.byref(adds)), "bp_msm_last_member_stats")
            out.append({"member": r, "upload_ms": u.value, "accumulate_ms": a.value, "device_ms": t.value, "mixed_adds": adds.value})
        return out

    def ntt(self, values, inverse=False, fmt=FR_MONT):
        """one vector; raises like the reference's assert!(is_power_of_two(n)) (utils.rs:65,108)"""
        a = _fr_array(values).copy()
        n = len(a)
        if n == 0 or n & (n - 1):
            raise BpError(-2, "ntt_381", "length %d is not a power of two" % n)
        self.check(self._lib.bp_ntt_fr(self._h, a.ctypes.data, n.bit_length() - 1, int(inverse), fmt, 1, n), "bp_ntt_fr")
        return a

    def ntt_batch(self, values, inverse=False, stride=None, fmt=FR_MONT):
        """values [batch, stride, 4]: transforms the first 2^k entries of every row (independent columns)"""
        a = np.ascontiguousarray(values, dtype=np.uint64).copy()
        assert a.ndim == 3 and a.shape[2] == 4
        batch, row = a.shape[0], a.shape[1]
        n = stride if stride is not None else row
        if n == 0 or n & (n - 1) or n > row:
            raise BpError(-2, "ntt_381", "length %d is not a power of two" % n)
        self.check(self._lib.bp_ntt_fr(self._h, a.ctypes.data, n.bit_length() - 1, int(inverse), fmt, batch, row), "bp_ntt_fr")
        return a

    def ntt_device(self, ptr, log_n, inverse=False, batch=1, stride=None):
        self.check(self._lib.bp_ntt_fr_device(self._h, ptr, log_n, int(inverse), batch, stride if stride else (1 << log_n)),
                   "bp_ntt_fr_device")

    def ntt_device_async(self, ptr, log_n, inverse=False, batch=1, stride=None):
        """enqueue only (bp_ntt_fr_device_async); synchronize() waits"""
        self.check(self._lib.bp_ntt_fr_device_async(self._h, ptr, log_n, int(inverse), batch, stride if stride else (1 << log_n)),
                   "bp_ntt_fr_device_async")

    def ntt_stats(self):
        ms, p = C.c_float(), C.c_uint32()
        self.check(self._lib.bp_ntt_last_stats(self._h, C.byref(ms), C.byref(p)), "bp_ntt_last_stats")
        return {"device_ms": ms.value, "passes": p.value, "members": self._lib.bp_ntt_last_members(self._h)}

    def poly_stats(self):
        """which path the last polynomial division took (bp_poly_last_stats): div_path 0 general, 1 binomial in one chunk, 2 plain
        carry, 3 workgroup carry, 4 segmented; chunks per chain; segments per chain (0 unless segmented)"""
        p, ch, g = C.c_uint32(), C.c_uint64(), C.c_uint32()
        self.check(self._lib.bp_poly_last_stats(self._h, C.byref(p), C.byref(ch), C.byref(g)), "bp_poly_last_stats")
        return {"div_path": p.value, "chunks": ch.value, "segments": g.value}

    def synthetic_scalars_device(self, ptr, n, seed):
        """fill HBM at `ptr` with n synthetic Montgomery scalars (the same stream the CPU baseline uses)"""
        self.check(self._lib.bp_fr_synthetic_device(self._h, ptr, n, seed), "bp_fr_synthetic_device")

    def _verify_args(self, what, vk, proofs, public_inputs, weights, challenges, fmt):
        """the arguments bp_verify_reduce and bp_verify_reduce_segments share, as arrays: (vk, records, m, publics, n_public, weights, challenges)"""
        if isinstance(vk, dict):
            vk = b"".join(vk[k] for k in CIRCUIT_COLUMNS)
        vkb = np.frombuffer(bytes(vk), dtype=np.uint8).copy()
        if len(vkb) != 768:
            raise BpError(-1, what, "vk: eight 96-byte commitments expected")
        rec, m = _proof_records(proofs)

        def scalars(a, per_proof, name):
            if a is None:
                return None, 0
            a = np.ascontiguousarray(a, dtype=np.uint64 if fmt == FR_MONT else np.uint8)
            width = 4 if fmt == FR_MONT else 32
            if a.size % width or (a.size // width) % max(m, 1) or (per_proof is not None and a.size != m * per_proof * width):
                raise BpError(-6, what, "%s: %d scalars do not fit %d proofs" % (name, a.size // width, m))
            return a, (a.size // width // m if m else 0)
        pub, n_public = scalars(public_inputs, None, "public_inputs")
        w, _ = scalars(weights, 1, "weights")
        ch, _ = scalars(challenges, 6, "challenges")
        return vkb, rec, m, pub, n_public, w, ch

    def verify_reduce(self, log_n, vk, proofs, public_inputs=None, weights=None, challenges=None, fmt=FR_MONT):
        """Verifier::verify (verifier.rs:80-192) of m proofs of one circuit up to the two pairings (bp_verify_reduce): returns
        (A96, B96); the batch is valid iff pairing(A, x_2) == pairing(B, G2 generator).  vk: the 768 bytes of
        Circuit.commitments (or that dict); proofs: m x 624 bytes (bytes, or a list of proofs); public_inputs: [m, n_public]
        scalars, row j = the vector handed to verify() for proof j; weights: m scalars drawn AFTER the proofs were received
        (None: a single proof, weight 1); challenges: None = the reference's transcript on the device, else [m, 6] scalars
        beta gamma alpha zeta nu mu.  Scalars: [.., 4] uint64 Montgomery limbs (fmt=FR_MONT) or [.., 32] uint8 canonical
        little-endian bytes (fmt=FR_BYTES_LE).  A rejected proof raises BpError whose `index` is the lowest failing proof."""
        vkb, rec, m, pub, n_public, w, ch = self._verify_args("verify_reduce", vk, proofs, public_inputs, weights, challenges, fmt)
        out, bad = np.zeros(192, dtype=np.uint8), C.c_size_t()
        rc = self._lib.bp_verify_reduce(self._h, log_n, vkb.ctypes.data, rec.ctypes.data if m else None, m,
                                        pub.ctypes.data if pub is not None and pub.size else None, n_public,
                                        None if w is None else w.ctypes.data, None if ch is None else ch.ctypes.data, fmt,
                                        out.ctypes.data, C.byref(bad))
        try:
            self.check(rc, "bp_verify_reduce")
        except BpError as e:
            e.index = bad.value if rc in (-3, -4) and bad.value != C.c_size_t(-1).value else None
            raise
        return out[:96].tobytes(), out[96:].tobytes()

    def verify_reduce_segments(self, log_n, vk, proofs, public_inputs=None, weights=None, challenges=None, fmt=FR_MONT, segment=1):
        """verify_reduce per segment of the batch (bp_verify_reduce_segments): a list of ceil(m / segment) pairs (A96, B96), pair s
        being what verify_reduce returns for the proofs [s * segment, (s + 1) * segment) alone.  segment=1: one pair per proof
        (weights may then be None: weight 1 each).  Arguments and errors as verify_reduce."""
        vkb, rec, m, pub, n_public, w, ch = self._verify_args("verify_reduce_segments", vk, proofs, public_inputs, weights, challenges, fmt)
        segment = int(segment)
        n_seg = -(-m // segment) if segment > 0 else 0
        out, bad = np.zeros(max(n_seg, 1) * 192, dtype=np.uint8), C.c_size_t()
        rc = self._lib.bp_verify_reduce_segments(self._h, log_n, vkb.ctypes.data, rec.ctypes.data if m else None, m,
                                                 pub.ctypes.data if pub is not None and pub.size else None, n_public,
                                                 None if w is None else w.ctypes.data, None if ch is None else ch.ctypes.data, fmt,
                                                 max(segment, 0), out.ctypes.data, C.byref(bad))
        try:
            self.check(rc, "bp_verify_reduce_segments")
        except BpError as e:
            e.index = bad.value if rc in (-3, -4) and bad.value != C.c_size_t(-1).value else None
            raise
        raw = out.tobytes()
        return [(raw[192 * s: 192 * s + 96], raw[192 * s + 96: 192 * s + 192]) for s in range(n_seg)]

    def verify_stats(self):
        """HIP-event milliseconds of the five stages of the last verify_reduce"""
        ms = (C.c_float * 5)()
        self.check(self._lib.bp_verify_last_stats(self._h, ms), "bp_verify_last_stats")
        return dict(zip(("upload_ms", "transcript_ms", "scalars_ms", "decode_check_ms", "msm_ms"), [float(v) for v in ms]))

    def verify_segments_stats(self):
        """HIP-event milliseconds of the last stage of the last verify_reduce_segments, in its three parts"""
        ms = (C.c_float * 3)()
        self.check(self._lib.bp_verify_segments_last_stats(self._h, ms), "bp_verify_segments_last_stats")
        return dict(zip(("mul_ms", "reduce_ms", "encode_ms"), [float(v) for v in ms]))

    def pairing_check(self, pairs, x_2, checks=0, gt=False):
        """bp_pairing_check: one pairing check per GPU lane; see the module function pairing_check"""
        return _pairing_check(self, pairs, x_2, checks, gt)

    def pairing_stats(self):
        """milliseconds of the three stages of the last pairing_check on this context"""
        ms = (C.c_float * 3)()
        self.check(self._lib.bp_pairing_last_stats(self._h, ms), "bp_pairing_last_stats")
        return dict(zip(("prepare_upload_ms", "miller_ms", "final_exp_ms"), [float(v) for v in ms]))

    def kzg_verify_reduce(self, commitments, z, ys, nu, proofs, weights=None, checks=0, fmt=FR_MONT):
        """bp_kzg_verify_reduce: m opening claims -> (A96, B96) with  batch holds  <=>  pairing(A, x_2) == pairing(B, G2 generator).
        commitments: m x count x 96 bytes (row i = claim i); z, nu, weights: [m] scalars; ys: [m, count] scalars; proofs: m x 96
        bytes; nu may be None with count == 1, weights with m <= 1.  Scalars as in verify_reduce.  checks=1 adds the subgroup test
        of every point.  A rejected claim raises BpError whose `index` is the lowest failing claim."""
        width, dt = (4, np.uint64) if fmt == FR_MONT else (32, np.uint8)
        rec = np.frombuffer(bytes(proofs), dtype=np.uint8).copy()
        com = np.frombuffer(bytes(commitments), dtype=np.uint8).copy()
        if len(rec) % 96 or len(com) % 96:
            raise BpError(-6, "kzg_verify_reduce", "points: 96-byte records expected")
        m = len(rec) // 96
        count = len(com) // 96 // m if m else 1
        if m and len(com) != m * count * 96:
            raise BpError(-6, "kzg_verify_reduce", "%d commitments do not fit %d claims" % (len(com) // 96, m))

        def scalars(a, n, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != n * width:
                raise BpError(-6, "kzg_verify_reduce", "%s: %d scalars expected" % (name, n))
            return a
        z, ys, nu, w = scalars(z, m, "z"), scalars(ys, m * count, "ys"), scalars(nu, m, "nu"), scalars(weights, m, "weights")
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        out, bad = np.zeros(192, dtype=np.uint8), C.c_size_t()
        rc = self._lib.bp_kzg_verify_reduce(self._h, ptr(com), m, count, ptr(z), ptr(ys), ptr(nu), ptr(rec), ptr(w), fmt, checks, out.ctypes.data,
                                            C.byref(bad))
        try:
            self.check(rc, "bp_kzg_verify_reduce")
        except BpError as e:
            e.index = bad.value if rc in (-3, -4) and bad.value != C.c_size_t(-1).value else None
            raise
        return out[:96].tobytes(), out[96:].tobytes()

    def kzg_stats(self):
        """milliseconds of the last Setup.open on this context (values and quotient; the commit) and of the last kzg_verify_reduce"""
        ms = (C.c_float * 3)()
        self.check(self._lib.bp_kzg_last_stats(self._h, ms), "bp_kzg_last_stats")
        return dict(zip(("values_quotient_ms", "commit_ms", "reduce_ms"), [float(v) for v in ms]))

    def kzg_open_all_stats(self):
        """milliseconds of the four stages of the last Setup.open_all on this context; table_ms is 0 when the table was there"""
        ms = (C.c_float * 4)()
        self.check(self._lib.bp_kzg_open_all_last_stats(self._h, ms), "bp_kzg_open_all_last_stats")
        return dict(zip(("table_ms", "field_ms", "toeplitz_ms", "final_ms"), [float(v) for v in ms]))

    def kzg_recover_stats(self):
        """milliseconds of the four stages of the last accepted recover_polynomial(_device) / Setup.recover_cells on this context;
        vanishing_ms and coset_ms are 0 when no cell was missing"""
        ms = (C.c_float * 4)()
        self.check(self._lib.bp_kzg_recover_last_stats(self._h, ms), "bp_kzg_recover_last_stats")
        return dict(zip(("vanishing_ms", "spread_ms", "coset_ms", "check_ms"), [float(v) for v in ms]))

    # ---- the structure of an SRS (capi_srs_check.hip) ----
    def srs_powers_reduce(self, handle, rho, first=0, n_pairs=None):
        """bp_srs_powers_reduce: (A96, B96) = (sum_i rho^i P_{first+i}, sum_i rho^i P_{first+i+1}) over n_pairs pairs (default: all
        from `first`); every pair is P_{i+1} = tau P_i exactly when pairing(A, x_2) == pairing(B, G2 generator).  rho: an integer
        the caller drew after the points were fixed, 128 bits of entropy or more"""
        n_pairs = self.srs_len(handle) - first - 1 if n_pairs is None else n_pairs
        r, out = _scalar32(rho), np.zeros(192, dtype=np.uint8)
        self.check(self._lib.bp_srs_powers_reduce(self._h, handle, first, n_pairs, r.ctypes.data, FR_BYTES_LE, out.ctypes.data), "bp_srs_powers_reduce")
        return out[:96].tobytes(), out[96:].tobytes()

    def srs_check_powers(self, handle, x_2, rho=None, generator=True):
        """bp_srs_check_powers: are the points the powers of the tau of x_2 (and, with generator=True, is P_0 the G1 generator)?
        None, or the lowest bad index: 0 for the generator, else the lowest i with P_i != tau P_{i-1} (1 for a wrong x_2).
        rho=None draws 128 bits here.  A rejected x_2 raises BpError"""
        x2 = np.frombuffer(bytes(x_2), dtype=np.uint8).copy()
        if len(x2) != 192:
            raise BpError(-6, "bp_srs_check_powers", "x_2: 192 bytes expected")
        r, bad = _scalar32(_draw_rho() if rho is None else rho), C.c_size_t()
        rc = self._lib.bp_srs_check_powers(self._h, handle, x2.ctypes.data, r.ctypes.data, FR_BYTES_LE, _lib.SRS_CHECK_GENERATOR if generator else 0,
                                           C.byref(bad))
        if rc == -3 and bad.value != _SIZE_MAX:
            return bad.value
        self.check(rc, "bp_srs_check_powers")
        return None

    def srs_check_stats(self):
        """reduces, host pairings and wall milliseconds of the last srs_check_powers / srs_adopt_lagrange on this context"""
        a, b, ms = C.c_uint32(), C.c_uint32(), C.c_float()
        self.check(self._lib.bp_srs_check_last_stats(self._h, C.byref(a), C.byref(b), C.byref(ms)), "bp_srs_check_last_stats")
        return {"reduces": a.value, "pairings": b.value, "ms": ms.value}

    def srs_adopt_lagrange(self, points, powers, log_n, rho=None):
        """bp_srs_adopt_lagrange: `points` (a loaded handle of 2^log_n points) checked against the first 2^log_n points of the
        powers-of-tau handle `powers` -- two MSMs and a transform, no pairing -- and returned as a NEW handle tagged Lagrange.
        Points that are not the Lagrange points raise BpError(BP_ERR_BAD_POINT) with the lowest wrong index in `index`"""
        r, h, bad = _scalar32(_draw_rho() if rho is None else rho), C.c_uint64(), C.c_size_t()
        rc = self._lib.bp_srs_adopt_lagrange(self._h, points, powers, log_n, r.ctypes.data, FR_BYTES_LE, C.byref(h), C.byref(bad))
        try:
            self.check(rc, "bp_srs_adopt_lagrange")
        except BpError as e:
            e.index = bad.value if rc == -3 and bad.value != _SIZE_MAX else None
            raise
        return h.value

    def srs_scale(self, handle, scalars=None, fmt=FR_MONT, device_ptr=None, n=None):
        """bp_srs_scale: a new SRS handle with points k_i P_i (same basis), one scalar per point: a host array ([n, 4] Montgomery
        limbs, or [n, 32] canonical bytes with fmt=FR_BYTES_LE) or (device_ptr, n).  The source is subgroup-tested first: a point
        outside raises BpError(BP_ERR_BAD_POINT) with its index in `index`"""
        h, bad = C.c_uint64(), C.c_size_t()
        if device_ptr is not None:
            rc = self._lib.bp_srs_scale(self._h, handle, device_ptr, n, fmt, 1, C.byref(h), C.byref(bad))
        else:
            k = _fr_array(scalars) if fmt == FR_MONT else np.ascontiguousarray(scalars, dtype=np.uint8).reshape(-1, 32)
            rc = self._lib.bp_srs_scale(self._h, handle, k.ctypes.data if len(k) else None, len(k), fmt, 0, C.byref(h), C.byref(bad))
        try:
            self.check(rc, "bp_srs_scale")
        except BpError as e:
            e.index = bad.value if rc == -3 and bad.value != _SIZE_MAX else None
            raise
        return h.value

    def srs_scale_stats(self):
        """HIP-event milliseconds of the last srs_scale on this context: subgroup test, multiplications, normalisation"""
        ms = (C.c_float * 3)()
        self.check(self._lib.bp_srs_scale_last_stats(self._h, ms), "bp_srs_scale_last_stats")
        return dict(zip(("subgroup_ms", "scale_ms", "normalise_ms"), [float(v) for v in ms]))

    def set_stream(self, stream_ptr):
        self.check(self._lib.bp_set_stream(self._h, stream_ptr), "bp_set_stream")

    def synchronize(self):
        self.check(self._lib.bp_synchronize(self._h), "bp_synchronize")
        self._async_keepalive.clear()


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def sum_partials(partials144):
    """host-side: add 144-byte projective partials and return the 96-byte affine encoding"""
    lib = _lib.load()
    buf = np.ascontiguousarray(np.frombuffer(bytes(partials144), dtype=np.uint8))
    out = np.zeros(96, dtype=np.uint8)
    rc = lib.bp_g1_sum_partials(buf.ctypes.data, len(buf) // 144, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "bp_g1_sum_partials")
    return bytes(out)


def combine_blobs(blobs):
    """host-side: the gathered MSM records of all ranks (n x MSM_BLOB_BYTES, host bytes) -> 96-byte affine encoding"""
    lib = _lib.load()
    buf = np.ascontiguousarray(np.frombuffer(bytes(blobs), dtype=np.uint8))
    assert len(buf) % _lib.MSM_BLOB_BYTES == 0
    out = np.zeros(96, dtype=np.uint8)
    rc = lib.bp_msm_blobs_combine(buf.ctypes.data, len(buf) // _lib.MSM_BLOB_BYTES, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "bp_msm_blobs_combine")
    return bytes(out)


def bytes96_to_partial(b96):
    lib = _lib.load()
    src, out = np.frombuffer(bytes(b96), dtype=np.uint8).copy(), np.zeros(144, dtype=np.uint8)
    rc = lib.bp_g1_bytes96_to_partial(src.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "bp_g1_bytes96_to_partial")
    return bytes(out)


def g2_mul_generator(k_int):
    """host-side: k * G2 as 192 bytes (G2Affine::to_uncompressed); x_2 of a setup is g2_mul_generator(tau) (setup.rs:20)"""
    out = np.zeros(192, dtype=np.uint8)
    if not 0 <= k_int < 1 << 256:
        raise BpError(-4, "bp_g2_mul_generator", "scalar outside 0 .. 2^256")
    k = np.frombuffer(int(k_int).to_bytes(32, "little"), dtype=np.uint8).copy()
    rc = _lib.load().bp_g2_mul_generator(k.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "bp_g2_mul_generator")
    return bytes(out)


def g2_mul(q192, k_int):
    """host-side: k * Q in G2 (bp_g2_mul), 192 bytes in and out; x_2 of a ceremony contribution is g2_mul(x_2, s)"""
    q = np.frombuffer(bytes(q192), dtype=np.uint8).copy()
    if len(q) != 192:
        raise BpError(-6, "bp_g2_mul", "192 bytes expected")
    k, out = _scalar32(k_int), np.zeros(192, dtype=np.uint8)
    rc = _lib.load().bp_g2_mul(q.ctypes.data, k.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "bp_g2_mul")
    return bytes(out)


def pairing_gt(p96, q192):
    """host-side: bls12_381::pairing(p, q) as the 576-byte memory image of Gt"""
    p, q = np.frombuffer(bytes(p96), dtype=np.uint8).copy(), np.frombuffer(bytes(q192), dtype=np.uint8).copy()
    if len(p) != 96 or len(q) != 192:
        raise BpError(-6, "bp_pairing_gt_host", "96 and 192 bytes expected")
    out = np.zeros(576, dtype=np.uint8)
    rc = _lib.load().bp_pairing_gt_host(p.ctypes.data, q.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "bp_pairing_gt_host")
    return bytes(out)


def _pairing_check(ctx, pairs, x_2, checks, gt):
    """ctx None: bp_pairing_check_host; else bp_pairing_check on that context"""
    if isinstance(pairs, (list, tuple)):
        pairs = b"".join(bytes(a) + bytes(b) for a, b in pairs)
    rec = np.frombuffer(bytes(pairs), dtype=np.uint8).copy()
    x2 = None if x_2 is None else np.frombuffer(bytes(x_2), dtype=np.uint8).copy()
    if len(rec) % 192 or x2 is None or len(x2) != 192:
        raise BpError(-6 if x2 is not None else -1, "pairing_check", "pairs: n x 192 bytes and x_2: 192 bytes expected")
    n = len(rec) // 192
    verdicts = np.zeros(max(n, 1), dtype=np.uint8)
    images = np.zeros(max(n, 1) * 576, dtype=np.uint8) if gt else None
    bad = C.c_size_t()
    args = (x2.ctypes.data, rec.ctypes.data if n else None, n, checks, verdicts.ctypes.data, None if images is None else images.ctypes.data, C.byref(bad))
    lib = _lib.load()
    rc = lib.bp_pairing_check_host(*args) if ctx is None else ctx._lib.bp_pairing_check(ctx._h, *args)
    if rc != 0:
        try:
            if ctx is None:
                raise BpError(rc, "bp_pairing_check_host")
            ctx.check(rc, "bp_pairing_check")
        except BpError as e:
            e.index = bad.value if rc == -3 and bad.value != C.c_size_t(-1).value else None
            raise
    out = [bool(v) for v in verdicts[:n]]
    if gt:
        raw = images.tobytes()
        return out, [raw[576 * i: 576 * i + 576] for i in range(n)]
    return out


def pairing_check(pairs, x_2, ctx=None, host=False, checks=0, gt=False):
    """n pairing checks against one setup: verdict i is pairing(A_i, x_2) == pairing(B_i, G2 generator).  pairs: n x 192 bytes
    A | B (what Verifier.pairing_inputs(_segments) returns, or a list of such pairs); x_2: 192 bytes.  host=True runs on the CPU
    (bp_pairing_check_host, no context needed), else one check per GPU lane on ctx (default: the default context).  checks: 1 adds
    the G1 subgroup test, 2 the G2 subgroup test of x_2.  gt=True returns (verdicts, images): the 576-byte Gt image per pair.
    A rejected point raises BpError with the lowest failing pair in `index`."""
    return _pairing_check(None if host else (ctx or default_context()), pairs, x_2, checks, gt)


# ------------------------------------------------------------------------------------------------
# reference-shaped API
# ------------------------------------------------------------------------------------------------
def root_of_unity(group_order, ctx=None):
    """utils.rs:39-43"""
    lib = _lib.load()
    out = np.zeros(4, dtype=np.uint64)
    rc = lib.bp_root_of_unity(group_order, FR_MONT, out.ctypes.data)
    if rc != 0:
        raise BpError(rc, "root_of_unity")
    return out


def roots_of_unity(group_order, ctx=None):
    """utils.rs:45-52"""
    ctx = ctx or default_context()
    out = np.zeros((group_order, 4), dtype=np.uint64)
    ctx.check(ctx._lib.bp_roots_of_unity(ctx._h, group_order, FR_MONT, out.ctypes.data), "roots_of_unity")
    return out


def ntt_381(elements, ctx=None):
    """utils.rs:63-81: natural-order DFT; asserts a power-of-two length"""
    return (ctx or default_context()).ntt(elements, inverse=False)


def i_ntt_381(elements, ctx=None):
    """utils.rs:106-129: inverse DFT including the 1/n factor"""
    return (ctx or default_context()).ntt(elements, inverse=True)


class BucketMSM:
    """src/msm.rs:8"""

    @staticmethod
    def bucket_msm(points96, scalars, b=256, c=4, ctx=None):
        """msm.rs:76-118.  points96: concatenated 96-byte encodings; scalars [n,4] Montgomery limbs.
        The reference walks floor(b / c) windows of c bits from the most significant end of the scalar's 256-bit image
        (msm.rs:83, 119-139): with b = 256 and c dividing 256 (its only call, setup.rs:36: b = 256, c = 4) that is the whole
        scalar; any other (b, c) silently drops the low 256 - c * floor(b / c) bits.  bp_msm_window_scalars reproduces exactly
        that (and the reference's panics as errors), so every (b, c) gives the reference's group element."""
        ctx = ctx or default_context()
        s = _fr_array(scalars)
        k = b // c if c > 0 else 0
        fmt = FR_MONT
        if not (0 < c <= 63 and k * c == 256):        # (c = 64 divides 256 too, but the reference's 1 << c bucket vector panics)
            eff = np.zeros((len(s), 32), dtype=np.uint8)
            rc = ctx._lib.bp_msm_window_scalars(s.ctypes.data, len(s), FR_MONT, b, c, eff.ctypes.data)
            if rc != 0:
                raise BpError(rc, "BucketMSM.bucket_msm", "the reference panics for b=%d, c=%d (msm.rs:24,105,132)" % (b, c))
            s, fmt = eff, FR_BYTES_LE
        h = ctx.srs_load(points96)
        try:
            return ctx.msm(h, s, fmt=fmt)
        finally:
            ctx.srs_free(h)


class _PolynomialOps:
    """The operators Polynomial and DevicePolynomial share (polynomial.rs:34-380, utils.rs:170-175).  A subclass says where its values
    live: _SUFFIX and _FMT (the suffix of its entry points' names and their scalar_fmt argument, if they take one), _ptr(),
    _alloc(n) -- a new polynomial of the same basis and context with room for n values -- and _cut(n), which keeps the first n."""

    def _same_kind(self, other):         # a Polynomial with a Polynomial, a DevicePolynomial with a DevicePolynomial (subclasses included)
        return isinstance(other, _PolynomialOps) and other._SUFFIX == self._SUFFIX

    def _call(self, name, fn, *args):
        c = self.ctx
        c.check(getattr(c._lib, fn + self._SUFFIX)(c._h, self._ptr(), len(self), *args), name)

    def _binop(self, other, fn, name, out_len):
        if self.basis != other.basis:
            raise BpError(-5, name, "Basis must be the same")
        out, n = self._alloc(out_len), C.c_size_t()
        self._call(name, fn, other._ptr(), len(other), self.basis, *self._FMT, out._ptr(), C.byref(n))
        out._cut(n.value)
        return out

    def _scalar(self, s, op, name):
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(4)
        out = self._alloc(len(self))
        self._call(name, "bp_poly_scalar_op", self.basis, s.ctypes.data, op, *self._FMT, out._ptr())
        return out

    def __add__(self, other):            # polynomial.rs:57-117
        if self._same_kind(other):
            return self._binop(other, "bp_poly_add", "Polynomial + Polynomial", max(len(self), len(other)))
        return self._scalar(other, 0, "Polynomial + Scalar")

    def __sub__(self, other):            # polynomial.rs:119-174
        if self._same_kind(other):
            return self._binop(other, "bp_poly_sub", "Polynomial - Polynomial", max(len(self), len(other)))
        return self._scalar(other, 1, "Polynomial - Scalar")

    def __mul__(self, other):            # polynomial.rs:176-312
        if self._same_kind(other):
            return self._binop(other, "bp_poly_mul", "Polynomial * Polynomial", len(self) + len(other))
        return self._scalar(other, 2, "Polynomial * Scalar")

    def __truediv__(self, other):        # polynomial.rs:314-380
        return self._binop(other, "bp_poly_div", "Polynomial / Polynomial", max(len(self), 1))

    def rlc(self, other, beta, gamma):   # impl Rlc for Polynomial (utils.rs:170-175): self + other * beta + gamma
        return self + other * beta + gamma

    def coeffs_evaluate(self, x):        # polynomial.rs:34-45
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(4)
        out = np.zeros(4, dtype=np.uint64)
        self._call("coeffs_evaluate", "bp_poly_evaluate", self.basis, x.ctypes.data, *self._FMT, out.ctypes.data)
        return out


class Polynomial(_PolynomialOps):
    """polynomial.rs:14-17; value semantics (every operator returns a new object)"""
    _SUFFIX, _FMT = "", (FR_MONT,)

    def __init__(self, values, basis, ctx=None):
        self.values = _fr_array(values).copy() if len(values) else np.zeros((0, 4), dtype=np.uint64)
        assert basis in (BASIS_LAGRANGE, BASIS_MONOMIAL)
        self.basis = basis
        self.ctx = ctx or default_context()

    def __len__(self):
        return len(self.values)

    def __eq__(self, other):
        return self.basis == other.basis and self.values.shape == other.values.shape and bool((self.values == other.values).all())

    def _ptr(self):
        return self.values.ctypes.data

    def _alloc(self, n):
        out = Polynomial((), self.basis, self.ctx)
        out.values = np.zeros((max(n, 1), 4), dtype=np.uint64)[:n]
        return out

    def _cut(self, n):
        self.values = self.values[:n]

    def ntt(self):                       # polynomial.rs:47-51
        if self.basis != BASIS_MONOMIAL:
            raise BpError(-5, "Polynomial.ntt", "needs the Monomial basis")
        return Polynomial(self.ctx.ntt(self.values, inverse=False), BASIS_LAGRANGE, self.ctx)

    def i_ntt(self):                     # polynomial.rs:52-55
        if self.basis != BASIS_LAGRANGE:
            raise BpError(-5, "Polynomial.i_ntt", "needs the Lagrange basis")
        return Polynomial(self.ctx.ntt(self.values, inverse=True), BASIS_MONOMIAL, self.ctx)

    def shift_left(self, n):             # polynomial.rs:22-33 (index permutation, host side)
        if self.basis != BASIS_LAGRANGE:
            raise BpError(-5, "Polynomial.shift_left", "needs the Lagrange basis")
        return np.roll(self.values, -(n % len(self)), axis=0)


class DevicePolynomial(_PolynomialOps):
    """polynomial.rs:14-17 with the coefficient / value vector resident in HBM (torch CUDA tensor, int64 [n, 4] =
    Montgomery limbs).  Same operators and rules as Polynomial; nothing but O(1) scalars crosses PCIe."""
    _SUFFIX, _FMT = "_device", ()

    def __init__(self, values, basis, ctx=None):
        import torch
        self.ctx = ctx or default_context()
        assert basis in (BASIS_LAGRANGE, BASIS_MONOMIAL)
        self.basis = basis
        if isinstance(values, torch.Tensor):
            self.t = values
        else:
            host = _fr_array(values) if len(values) else np.zeros((0, 4), dtype=np.uint64)
            self.t = torch.from_numpy(host.view(np.int64).copy()).to(torch.device("cuda", self.ctx.device))
            torch.cuda.current_stream().synchronize()

    @staticmethod
    def empty(n, basis, ctx):
        import torch
        return DevicePolynomial(torch.empty((max(n, 1), 4), dtype=torch.int64, device=torch.device("cuda", ctx.device))[:n], basis, ctx)

    def __len__(self):
        return self.t.shape[0]

    @property
    def values(self):
        return self.t.cpu().numpy().view(np.uint64)

    def _ptr(self):
        return self.t.data_ptr() if len(self) else 0

    def _alloc(self, n):
        return DevicePolynomial.empty(n, self.basis, self.ctx)

    def _cut(self, n):
        self.t = self.t[:n]

    def _transform(self, inverse, need, to):
        if self.basis != need:
            raise BpError(-5, "Polynomial.ntt/i_ntt", "wrong basis")
        n = len(self)
        if n == 0 or n & (n - 1):
            raise BpError(-2, "ntt_381", "length %d is not a power of two" % n)
        out = DevicePolynomial(self.t.clone(), to, self.ctx)
        import torch
        torch.cuda.current_stream().synchronize()
        self.ctx.ntt_device(out._ptr(), n.bit_length() - 1, inverse=inverse)
        return out

    def ntt(self):
        return self._transform(False, BASIS_MONOMIAL, BASIS_LAGRANGE)

    def i_ntt(self):
        return self._transform(True, BASIS_LAGRANGE, BASIS_MONOMIAL)

    def scale_powers(self, w):
        """p(x) -> p(w x)  (prover.rs:661-674)"""
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(4)
        out = DevicePolynomial.empty(len(self), self.basis, self.ctx)
        c = self.ctx
        c.check(c._lib.bp_poly_scale_powers_device(c._h, self._ptr(), len(self), w.ctypes.data, out._ptr()), "scale_powers")
        return out

    def slice(self, lo, hi=None):
        return DevicePolynomial(self.t[lo:hi].contiguous(), self.basis, self.ctx)


def _recover_args(name, indices, cell_size, group_order, n_coeffs):
    """(log_n, log_l, the indices as uint32, n_coeffs) of a recovery; n_coeffs=None is group_order // 2"""
    log_n, log_l = Setup._cell_logs(name, group_order, cell_size)
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    if ((idx < 0) | (idx >= 1 << 32)).any():
        raise BpError(-1, name, "a cell index outside 0 .. 2^32")
    return log_n, log_l, idx.astype(np.uint32), max(group_order // 2, 1) if n_coeffs is None else int(n_coeffs)


def _recover_check(ctx, rc, bad, name):
    """raise for rc != 0 with `index` = first_bad: the position in `indices` (a bad or repeated index, a value >= q) or, for
    BP_ERR_ASSERT, the lowest non-zero coefficient index of the interpolant"""
    try:
        ctx.check(rc, name)
    except BpError as e:
        e.index = bad.value if bad.value != _SIZE_MAX else None
        raise


def recover_polynomial(indices, cells, group_order, n_coeffs=None, ctx=None, fmt=FR_MONT):
    """the polynomial of fewer than n_coeffs coefficients that takes the given cells (bp_kzg_recover): a Monomial Polynomial of n_coeffs
    coefficients.  indices: m distinct cell indices in any order; cells: [m, l, 4] uint64 Montgomery limbs (fmt=FR_MONT) or
    [m, l, 32] uint8 canonical little-endian bytes (FR_BYTES_LE), cells[i] being cell indices[i] of the domain of group_order points in
    the cell order of Setup.open_cosets.  n_coeffs=None means group_order // 2, the rate-1/2 extension of a data-availability column.
    Needs m * l >= n_coeffs.  With m * l > n_coeffs the cells are checked against each other: BpError BP_ERR_ASSERT (index = the
    lowest non-zero coefficient of their interpolant) if no such polynomial exists.  With m * l == n_coeffs there is NOTHING to check:
    the interpolant of whatever was given comes back.  Other errors carry the position in `indices` in `index`."""
    c = ctx or default_context()
    width, dt = (4, np.uint64) if fmt == FR_MONT else (32, np.uint8)
    v = np.ascontiguousarray(cells, dtype=dt)
    if v.ndim != 3 or v.shape[2] != width or v.shape[0] != len(indices):
        raise BpError(-6, "recover_polynomial", "cells: [m, l, %d] expected" % width)
    log_n, log_l, idx, d = _recover_args("recover_polynomial", indices, v.shape[1], group_order, n_coeffs)
    out, bad = np.zeros((min(max(d, 1), group_order), 4), dtype=np.uint64), C.c_size_t(-1)      # d > group_order is refused before a write
    rc = c._lib.bp_kzg_recover(c._h, log_n, log_l, idx.ctypes.data, v.ctypes.data, len(idx), d, fmt, out.ctypes.data, C.byref(bad))
    _recover_check(c, rc, bad, "recover_polynomial")
    if fmt != FR_MONT:
        out = scalars_from_ints([int.from_bytes(out[i].tobytes(), "little") for i in range(d)])
    return Polynomial(out[:d], BASIS_MONOMIAL, c)


def recover_polynomial_device(indices, d_cells, cell_size, group_order, n_coeffs=None, ctx=None):
    """recover_polynomial with the cells in HBM (bp_kzg_recover_device): d_cells is a torch int64 tensor of m * cell_size Montgomery
    scalars ([m, l, 4] or [m * l, 4]) on the context's device.  Returns a Monomial DevicePolynomial of n_coeffs coefficients, a view of a
    buffer of group_order scalars whose other places are zero (`.t._base` keeps it alive)."""
    import torch
    c = ctx or default_context()
    log_n, log_l, idx, d = _recover_args("recover_polynomial_device", indices, cell_size, group_order, n_coeffs)
    t = d_cells.contiguous()
    if t.dtype != torch.int64 or t.numel() != len(idx) * cell_size * 4:
        raise BpError(-6, "recover_polynomial_device", "d_cells: %d x %d Montgomery scalars (int64 limbs) expected" % (len(idx), cell_size))
    out = torch.empty((group_order, 4), dtype=torch.int64, device=torch.device("cuda", c.device))
    torch.cuda.current_stream().synchronize()
    bad = C.c_size_t(-1)
    rc = c._lib.bp_kzg_recover_device(c._h, log_n, log_l, idx.ctypes.data, t.data_ptr(), len(idx), d, out.data_ptr(), C.byref(bad))
    _recover_check(c, rc, bad, "recover_polynomial_device")
    return DevicePolynomial(out[:d], BASIS_MONOMIAL, c)


def commit_device(setup, poly):
    """Setup::commit (setup.rs:32-37) of an HBM-resident polynomial"""
    c = setup.ctx
    out = np.zeros(96, dtype=np.uint8)
    c.check(c._lib.bp_commit_device(c._h, setup.handle, poly._ptr(), len(poly), poly.basis, out.ctypes.data), "Setup.commit")
    return bytes(out)


def commit_many_device(setup, polys):
    """several Setup::commit calls in one (bp_commit_many_device): the pipelines of the commitments overlap"""
    c = setup.ctx
    k = len(polys)
    if k == 0:
        return []
    ptrs = (C.c_void_p * k)(*[p._ptr() for p in polys])
    lens = (C.c_size_t * k)(*[len(p) for p in polys])
    out = np.zeros(96 * k, dtype=np.uint8)
    c.check(c._lib.bp_commit_many_device(c._h, setup.handle, ptrs, lens, k, polys[0].basis, out.ctypes.data), "Setup.commit (many)")
    return [bytes(out[96 * i: 96 * (i + 1)]) for i in range(k)]


def round_2_z_device(a, b, c, s1, s2, s3, beta, gamma, k1=None, k2=None):
    """prover.rs:279-319 on DevicePolynomial columns -> DevicePolynomial (Lagrange)"""
    ctx = a.ctx
    n = len(a)
    k1 = scalar_from_int(2) if k1 is None else np.ascontiguousarray(k1, dtype=np.uint64)
    k2 = scalar_from_int(3) if k2 is None else np.ascontiguousarray(k2, dtype=np.uint64)
    beta, gamma = np.ascontiguousarray(beta, dtype=np.uint64), np.ascontiguousarray(gamma, dtype=np.uint64)
    out = DevicePolynomial.empty(n, BASIS_LAGRANGE, ctx)
    ctx.check(ctx._lib.bp_grand_product_device(ctx._h, a._ptr(), b._ptr(), c._ptr(), s1._ptr(), s2._ptr(), s3._ptr(), n, beta.ctypes.data,
                                               gamma.ctypes.data, k1.ctypes.data, k2.ctypes.data, out._ptr()), "round_2 grand product")
    return out


def roots_of_unity_device(n, ctx=None):
    ctx = ctx or default_context()
    out = DevicePolynomial.empty(n, BASIS_LAGRANGE, ctx)
    ctx.check(ctx._lib.bp_roots_of_unity_device(ctx._h, n, out._ptr()), "roots_of_unity")
    return out


def round_2_z(a, b, c, s1, s2, s3, beta, gamma, k1=None, k2=None, ctx=None):
    """prover.rs:279-319: Lagrange values z_0..z_{n-1} of the permutation grand product (raises where the reference panics)"""
    ctx = ctx or default_context()
    cols = [_fr_array(x) for x in (a, b, c, s1, s2, s3)]
    n = len(cols[0])
    assert all(len(x) == n for x in cols)
    k1 = scalar_from_int(2) if k1 is None else np.ascontiguousarray(k1, dtype=np.uint64)
    k2 = scalar_from_int(3) if k2 is None else np.ascontiguousarray(k2, dtype=np.uint64)
    beta, gamma = np.ascontiguousarray(beta, dtype=np.uint64), np.ascontiguousarray(gamma, dtype=np.uint64)
    out = np.zeros((n, 4), dtype=np.uint64)
    ctx.check(ctx._lib.bp_grand_product(ctx._h, *[x.ctypes.data for x in cols], n, beta.ctypes.data, gamma.ctypes.data, k1.ctypes.data,
                                        k2.ctypes.data, FR_MONT, out.ctypes.data), "round_2 grand product")
    return out


class Setup:
    """src/setup.rs:7-10: the powers of tau in G1, resident on the GPU, and x_2 = tau * G2 as 192 bytes (None when the setup was
    loaded from G1 points alone and no x_2= was given: the verdict methods of Verifier then raise).
    A Setup serves every commitment of a prover, so it builds the SRS's fixed-base window tables once
    (bp_srs_precompute) unless tables=False or BP_SRS_TABLES=0."""

    def __init__(self, handle, ctx, tables=True, x_2=None):
        self.handle, self.ctx, self.tables_error = handle, ctx, None
        self.x_2 = None if x_2 is None else bytes(x_2)
        if self.x_2 is not None and len(self.x_2) != 192:
            raise BpError(-6, "Setup", "x_2: 192 bytes expected")
        if tables and os.environ.get("BP_SRS_TABLES", "1") != "0":
            try:
                ctx.srs_precompute(handle, 0)
            except BpError as e:          # tables are an optimisation (they need windows x 128 B per point of HBM): commits work without
                self.tables_error = e

    @staticmethod
    def generate_srs(powers, tau_int, ctx=None, tables=True):
        """setup.rs:12-31: [G, tau G, ..., tau^(powers-1) G], generated and kept on the GPU"""
        ctx = ctx or default_context()
        return Setup(ctx.srs_generate(powers, tau_int), ctx, tables, g2_mul_generator(tau_int % Q))

    @staticmethod
    def from_points(points96, ctx=None, tables=True, x_2=None):
        ctx = ctx or default_context()
        return Setup(ctx.srs_load(points96), ctx, tables, x_2)

    @staticmethod
    def from_compressed(points48, ctx=None, tables=True, check_subgroup=True, x_2=None):
        """a ceremony's SRS: 48-byte compressed records, decoded (and by default subgroup-checked) on the GPU"""
        ctx = ctx or default_context()
        return Setup(ctx.srs_load_compressed48(points48, check_subgroup), ctx, tables, x_2)

    def powers_of_x(self):
        return self.ctx.srs_export(self.handle)

    def powers_of_x_compressed(self):
        return self.ctx.srs_export_compressed48(self.handle)

    @property
    def basis(self):
        """BASIS_MONOMIAL (powers of tau), or BASIS_LAGRANGE for a Setup made by lagrange()"""
        return self.ctx.srs_basis(self.handle)[0]

    def lagrange(self, group_order, tables=True):
        """the Setup over [L_i(tau)] G for the group_order-th roots of unity (a power of two, at most the number of powers): same
        context, same x_2.  Its commit / commit_device / commit_many_device take Lagrange polynomials of group_order values --
        the same commitment as committing their i_ntt() to this Setup, with no transform in front of the MSM."""
        if group_order < 1 or group_order & (group_order - 1):
            raise BpError(-2, "Setup.lagrange", "group_order %d is not a power of two" % group_order)
        return Setup(self.ctx.srs_lagrange(self.handle, group_order.bit_length() - 1), self.ctx, tables, self.x_2)

    def check_powers(self, rho=None, generator=True):
        """are the points G, tau G, tau^2 G, ... for the tau of x_2?  (bp_srs_check_powers: one random linear combination, two
        MSMs, one host pairing check; a failure is located by bisection.)  None, or the lowest bad index -- 0: P_0 is not the
        generator (generator=True), i >= 1: P_i != tau P_{i-1}.  rho=None draws 128 bits with the top bit set."""
        if self.x_2 is None:
            raise BpError(-1, "Setup.check_powers", "the setup has no x_2 (pass x_2= to Setup.from_points / from_compressed)")
        return self.ctx.srs_check_powers(self.handle, self.x_2, rho, generator)

    @staticmethod
    def from_lagrange_points(points, powers_setup, rho=None, tables=True, compressed=False):
        """a Lagrange-basis Setup from SHIPPED Lagrange points (96-byte records, or 48-byte ones with compressed=True; a power of
        two of them), adopted only after they were checked against powers_setup's powers (bp_srs_adopt_lagrange: no pairing).
        Same context and x_2 as powers_setup.  Wrong points raise BpError(BP_ERR_BAD_POINT) with the lowest wrong index in `index`."""
        ctx = powers_setup.ctx
        n = len(bytes(points)) // (48 if compressed else 96)
        if n < 1 or n & (n - 1):
            raise BpError(-2, "Setup.from_lagrange_points", "%d points: not a power of two" % n)
        loaded = ctx.srs_load_compressed48(points) if compressed else ctx.srs_load(points)
        try:
            h = ctx.srs_adopt_lagrange(loaded, powers_setup.handle, n.bit_length() - 1, rho)
        finally:
            ctx.srs_free(loaded)
        return Setup(h, ctx, tables, powers_setup.x_2)

    def contribute(self, s_int, tables=True):
        """one contribution to the ceremony: a new Setup with points s^i P_i and x_2' = s x_2 (bp_srs_scale, one multiplication
        per GPU lane; the scalars s^i are made on the device).  The secret s is the caller's to forget."""
        import torch
        s_int, c, n = int(s_int) % Q, self.ctx, self.ctx.srs_len(self.handle)
        ones = DevicePolynomial(np.tile(scalar_from_int(1), (n, 1)), BASIS_MONOMIAL, c)
        pows = ones.scale_powers(scalar_from_int(s_int))
        torch.cuda.current_stream().synchronize()
        h = c.srs_scale(self.handle, device_ptr=pows._ptr(), n=n)
        return Setup(h, c, tables, None if self.x_2 is None else g2_mul(self.x_2, s_int))

    def verify_contribution(self, previous, s_2):
        """is this Setup `previous` after ONE contribution whose secret s the contributor published as s_2 = s G2?  The lengths
        are equal, this Setup is a clean powers-of-tau SRS (check_powers), and pairing(P'_1, G2) == pairing(P_1, s_2)."""
        n = self.ctx.srs_len(self.handle)
        if n != previous.ctx.srs_len(previous.handle) or n < 2 or self.check_powers() is not None:
            return False
        p1, q1 = previous.ctx.srs_export(previous.handle, 1, 1), self.ctx.srs_export(self.handle, 1, 1)
        return pairing_check([(p1, q1)], s_2, host=True)[0]

    def commit(self, polynomial):
        """setup.rs:32-37: asserts the Monomial basis, then bucket_msm over the whole SRS (a Setup made by lagrange(): asserts the
        Lagrange basis and the length)"""
        c = self.ctx
        out = np.zeros(96, dtype=np.uint8)
        c.check(c._lib.bp_commit(c._h, self.handle, polynomial.values.ctypes.data, len(polynomial), polynomial.basis, FR_MONT,
                                 out.ctypes.data), "Setup.commit")
        return bytes(out)

    def commit_device(self, polynomial):
        return commit_device(self, polynomial)

    def commit_many_device(self, polynomials):
        return commit_many_device(self, polynomials)

    def open(self, polys, z, nu=None):
        """KZG opening of one polynomial, or of a list of up to 16 (all Polynomial or all DevicePolynomial), at the point z
        (bp_kzg_open / bp_kzg_open_device): returns (ys, W96) -- ys [count, 4] the values f_j(z), W96 the ONE proof for
        sum_j nu^j f_j.  The polynomials must be in this Setup's basis: Monomial against the powers of tau, Lagrange (group_order
        values, never transformed) against a Setup made by lagrange().  z, nu: Montgomery limbs; nu may be None for one polynomial."""
        ps = [polys] if isinstance(polys, _PolynomialOps) else list(polys)
        if not ps or any(not ps[0]._same_kind(p) or p.basis != ps[0].basis for p in ps):
            raise BpError(-1, "Setup.open", "one kind and one basis of polynomial expected (and at least one)")
        c, k = self.ctx, len(ps)
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(4)
        nu = None if nu is None else np.ascontiguousarray(nu, dtype=np.uint64).reshape(4)
        ptrs = (C.c_void_p * k)(*[p._ptr() if len(p) else None for p in ps])
        lens = (C.c_size_t * k)(*[len(p) for p in ps])
        ys, w = np.zeros((k, 4), dtype=np.uint64), np.zeros(96, dtype=np.uint8)
        fn = getattr(c._lib, "bp_kzg_open" + ps[0]._SUFFIX)
        c.check(fn(c._h, self.handle, ptrs, lens, k, ps[0].basis, z.ctypes.data, None if nu is None else nu.ctypes.data, FR_MONT,
                   ys.ctypes.data, w.ctypes.data), "Setup.open")
        return ys, bytes(w)

    def prepare_open_all(self, group_order):
        """build and keep the table open_all needs for this group_order (bp_srs_open_all_prepare: 2 * group_order points of HBM,
        freed with the SRS; another group_order replaces it).  Optional: open_all builds it on first use."""
        if group_order < 1 or group_order & (group_order - 1):
            raise BpError(-2, "Setup.prepare_open_all", "group_order %d is not a power of two" % group_order)
        c = self.ctx
        c.check(c._lib.bp_srs_open_all_prepare(c._h, self.handle, group_order.bit_length() - 1), "Setup.prepare_open_all")

    def open_all(self, poly, group_order=None):
        """ALL group_order KZG proofs of one Polynomial or DevicePolynomial on its domain, in one call (bp_kzg_open_all /
        bp_kzg_open_all_device): returns (ys [n, 4] uint64, proofs [n, 96] uint8) with ys[i] = f(w^i) and proofs[i] the proof of
        that opening, w = root_of_unity(n).  A Monomial polynomial has at most n coefficients (group_order=None: the next power of
        two), a Lagrange one exactly n values; this Setup must hold the powers of tau (n - 1 of them or more).  Claim i is then
        Opening(commitment, w^i, ys[i:i+1], None, bytes(proofs[i]))."""
        c = self.ctx
        n = group_order
        if n is None:
            n = len(poly) if poly.basis == BASIS_LAGRANGE else max(1, 1 << max(len(poly) - 1, 0).bit_length())
        if n < 1 or n & (n - 1):
            raise BpError(-2, "Setup.open_all", "group_order %d is not a power of two" % n)
        ys, proofs = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 96), dtype=np.uint8)
        head = (c._h, self.handle, poly._ptr() if len(poly) else None, len(poly), poly.basis)
        fn = getattr(c._lib, "bp_kzg_open_all" + poly._SUFFIX)
        c.check(fn(*head, *poly._FMT, n.bit_length() - 1, ys.ctypes.data, proofs.ctypes.data), "Setup.open_all")
        return ys, proofs

    def opening_pairing_inputs(self, openings, weights=None, checks=0):
        """the claims of a list of Opening records (one polynomial count for all) reduced to (A96, B96): they hold iff
        pairing(A, x_2) == pairing(B, G2 generator).  weights: one scalar per claim, drawn after the claims were received, >= 128
        bits of entropy each (None: a single claim).  checks=1 adds the subgroup test of every commitment and proof."""
        openings = [openings] if isinstance(openings, Opening) else list(openings)
        com = []
        for o in openings:
            cs = [o.commitments] if isinstance(o.commitments, (bytes, bytearray)) else list(o.commitments)
            com.append(b"".join(bytes(x) for x in cs))
        if len(set(len(x) for x in com)) > 1:
            raise BpError(-6, "Setup.opening_pairing_inputs", "every claim must open the same number of polynomials")
        m = len(openings)
        limbs = lambda vals, n: np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.uint64).reshape(n, 4) for v in vals])) if m else np.zeros((0, 4), np.uint64)
        count = len(com[0]) // 96 if m else 1
        has_nu = [o.nu is not None for o in openings]
        if m and any(has_nu) != all(has_nu):
            raise BpError(-1, "Setup.opening_pairing_inputs", "nu: given for every claim or for none")
        nu = limbs([o.nu for o in openings], 1) if m and all(has_nu) else None
        return self.ctx.kzg_verify_reduce(b"".join(com), limbs([o.z for o in openings], 1), limbs([o.ys for o in openings], count), nu,
                                          b"".join(bytes(o.proof) for o in openings), weights, checks)

    def verify_openings(self, openings, weights=None, host=True):
        """do the claims hold against this Setup's x_2?  opening_pairing_inputs, then one pairing check, on the host or on the
        GPU.  weights=None with several claims draws 128-bit weights here (the claims are in hand by then)."""
        if self.x_2 is None:
            raise BpError(-1, "Setup.verify_openings", "the setup has no x_2 (pass x_2= to Setup.from_points / from_compressed)")
        openings = [openings] if isinstance(openings, Opening) else list(openings)
        if weights is None and len(openings) > 1:
            import secrets
            weights = scalars_from_ints([secrets.randbits(128) | 1 << 127 for _ in openings])
        pair = self.opening_pairing_inputs(openings, weights)
        return pairing_check([pair], self.x_2, ctx=self.ctx, host=host)[0]


    # ---- cell proofs: one proof per coset of cell_size points (bp_kzg_open_cosets, bp_kzg_verify_cells_reduce) ----
    @staticmethod
    def _cell_logs(name, group_order, cell_size):
        for what, v in (("group_order", group_order), ("cell_size", cell_size)):
            if v < 1 or v & (v - 1):
                raise BpError(-2, name, "%s %d is not a power of two" % (what, v))
        return group_order.bit_length() - 1, cell_size.bit_length() - 1

    def prepare_open_cosets(self, group_order, cell_size):
        """build and keep the table open_cosets needs for (group_order, cell_size) (bp_srs_open_cosets_prepare: 2 * group_order
        points of HBM in the ONE table slot of this SRS, which prepare_open_all / open_all use with cell_size 1: another key
        replaces the table).  Optional: open_cosets builds it on first use."""
        log_n, log_l = self._cell_logs("Setup.prepare_open_cosets", group_order, cell_size)
        c = self.ctx
        c.check(c._lib.bp_srs_open_cosets_prepare(c._h, self.handle, log_n, log_l), "Setup.prepare_open_cosets")

    def open_cosets(self, poly, cell_size, group_order=None):
        """the group_order / cell_size CELL proofs of one Polynomial or DevicePolynomial in one call (bp_kzg_open_cosets /
        bp_kzg_open_cosets_device): returns (cells [r, l, 4] uint64, proofs [r, 96] uint8), r = n / l.  Cell k is the coset
        {w^(k + r j) : j < l} of the domain, cells[k, j] = f(w^(k + r j)), and proofs[k] = [q_k(tau)] G with
        q_k = f div (x^l - w^(k l)) is its ONE proof.  Polynomial and Setup as for open_all (the first n - l points are used).
        Claim k is then CellOpening(commitment, k, cells[k], bytes(proofs[k])).  cell_size == 1 is open_all."""
        c = self.ctx
        n = group_order
        if n is None:
            n = len(poly) if poly.basis == BASIS_LAGRANGE else max(1, 1 << max(len(poly) - 1, 0).bit_length())
            n = max(n, cell_size)
        log_n, log_l = self._cell_logs("Setup.open_cosets", n, cell_size)
        r = max(n // cell_size, 1)
        cells, proofs = np.zeros((r, cell_size, 4), dtype=np.uint64), np.zeros((r, 96), dtype=np.uint8)
        head = (c._h, self.handle, poly._ptr() if len(poly) else None, len(poly), poly.basis)
        fn = getattr(c._lib, "bp_kzg_open_cosets" + poly._SUFFIX)
        c.check(fn(*head, *poly._FMT, log_n, log_l, cells.ctypes.data, proofs.ctypes.data), "Setup.open_cosets")
        return cells, proofs

    def recover_cells(self, indices, cells, group_order, n_coeffs=None):
        """ALL group_order / cell_size cells and cell proofs of a column from m of its cells (bp_kzg_recover_cells: recover_polynomial,
        then open_cosets on the coefficients where they lie, in HBM): returns (cells [r, l, 4] uint64, proofs [r, 96] uint8), the
        shapes of open_cosets, the given cells among them as they were given.  indices, cells ([m, l, 4] Montgomery limbs), n_coeffs
        (None: group_order // 2) and the errors are recover_polynomial's; the Setup is open_cosets' (the first n - l powers of tau)."""
        c = self.ctx
        v = np.ascontiguousarray(cells, dtype=np.uint64)
        if v.ndim != 3 or v.shape[2] != 4 or v.shape[0] != len(indices):
            raise BpError(-6, "Setup.recover_cells", "cells: [m, l, 4] expected")
        l = v.shape[1]
        log_n, log_l, idx, d = _recover_args("Setup.recover_cells", indices, l, group_order, n_coeffs)
        r = max(group_order // l, 1)
        out, proofs, bad = np.zeros((r, l, 4), dtype=np.uint64), np.zeros((r, 96), dtype=np.uint8), C.c_size_t(-1)
        rc = c._lib.bp_kzg_recover_cells(c._h, self.handle, log_n, log_l, idx.ctypes.data, v.ctypes.data, len(idx), d, FR_MONT, out.ctypes.data,
                                         proofs.ctypes.data, C.byref(bad))
        _recover_check(c, rc, bad, "Setup.recover_cells")
        return out, proofs

    def cell_pairing_inputs(self, claims, group_order, weights=None, checks=0):
        """the claims of a list of CellOpening records (one cell size for all) reduced to (A96, B96): they hold iff
        pairing(A, [tau^cell_size]_2) == pairing(B, G2 generator) (bp_kzg_verify_cells_reduce).  weights: one scalar per claim,
        drawn after the claims were received, >= 128 bits of entropy each (None: a single claim).  checks=1 adds the subgroup
        test of every commitment and proof.  A rejected claim raises BpError with the lowest failing claim in `index`."""
        claims = [claims] if isinstance(claims, CellOpening) else list(claims)
        m = len(claims)
        vals = [np.ascontiguousarray(o.values, dtype=np.uint64).reshape(-1, 4) for o in claims]
        if len(set(len(v) for v in vals)) > 1:
            raise BpError(-6, "Setup.cell_pairing_inputs", "every claim must have the same number of values")
        l = len(vals[0]) if m else 1
        log_n, log_l = self._cell_logs("Setup.cell_pairing_inputs", group_order, l)
        com = np.frombuffer(b"".join(bytes(o.commitment) for o in claims), dtype=np.uint8).copy()
        rec = np.frombuffer(b"".join(bytes(o.proof) for o in claims), dtype=np.uint8).copy()
        if len(com) != 96 * m or len(rec) != 96 * m:
            raise BpError(-6, "Setup.cell_pairing_inputs", "points: 96-byte records expected")
        idx = np.array([o.index for o in claims], dtype=np.uint32)
        v = np.ascontiguousarray(np.stack(vals)) if m else np.zeros((0, 4), np.uint64)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
        if w is not None and w.size != 4 * m:
            raise BpError(-6, "Setup.cell_pairing_inputs", "weights: %d scalars expected" % m)
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        c, out, bad = self.ctx, np.zeros(192, dtype=np.uint8), C.c_size_t(-1)
        rc = c._lib.bp_kzg_verify_cells_reduce(c._h, self.handle, log_n, log_l, ptr(com), ptr(idx), ptr(v), ptr(rec), m, ptr(w), FR_MONT, checks,
                                               out.ctypes.data, C.byref(bad))
        try:
            c.check(rc, "bp_kzg_verify_cells_reduce")
        except BpError as e:
            e.index = bad.value if rc in (-1, -3, -4) and bad.value != C.c_size_t(-1).value else None
            raise
        return out[:96].tobytes(), out[96:].tobytes()

    def verify_cells(self, claims, group_order, tau_l_g2, weights=None, host=True):
        """do the cell claims hold?  cell_pairing_inputs, then one pairing check against tau_l_g2 = [tau^cell_size]_2 (192 bytes,
        the CALLER'S: a ceremony ships the G2 powers), on the host or on the GPU.  weights=None with several claims draws
        128-bit weights here (the claims are in hand by then)."""
        claims = [claims] if isinstance(claims, CellOpening) else list(claims)
        if weights is None and len(claims) > 1:
            import secrets
            weights = scalars_from_ints([secrets.randbits(128) | 1 << 127 for _ in claims])
        pair = self.cell_pairing_inputs(claims, group_order, weights)
        return pairing_check([pair], tau_l_g2, ctx=self.ctx, host=host)[0]


CellOpening = collections.namedtuple("CellOpening", "commitment index values proof")
CellOpening.__doc__ = """one KZG cell claim: `commitment` (96 bytes) takes the values `values` ([l, 4], cell order) on cell `index` of its
domain, with the proof `proof` (96 bytes) -- what Setup.commit and Setup.open_cosets return, put together"""

Opening = collections.namedtuple("Opening", "commitments z ys nu proof")
Opening.__doc__ = """one KZG claim: `commitments` (96 bytes, or a list of them) open at `z` to the values `ys` ([count, 4]), combined by
`nu` (None for one polynomial), with the proof `proof` (96 bytes) -- what Setup.commit and Setup.open return, put together"""


CIRCUIT_COLUMNS = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")


class Circuit:
    """CommonPreprocessedInput (src/program.rs:34-50) resident in HBM: the eight Lagrange columns QL QR QM QO QC S1 S2 S3
    of a 2^log_n-row circuit, uploaded once (bp_circuit_load)"""

    def __init__(self, columns, ctx=None):
        self.ctx = ctx or default_context()
        cols = [_fr_array(columns[k]) for k in CIRCUIT_COLUMNS] if isinstance(columns, dict) else [_fr_array(c) for c in columns]
        n = len(cols[0])
        if len(cols) != 8 or any(len(c) != n for c in cols) or n < 8 or n & (n - 1):
            raise BpError(-2, "Circuit", "eight columns of equal power-of-two length >= 8 expected")
        self.group_order = n
        ptrs = (C.c_void_p * 8)(*[c.ctypes.data for c in cols])
        h = C.c_uint64()
        self.ctx.check(self.ctx._lib.bp_circuit_load(self.ctx._h, n.bit_length() - 1, ptrs, FR_MONT, 0, C.byref(h)), "bp_circuit_load")
        self.handle = h.value

    @classmethod
    def from_wires(cls, selectors, wire_ids, n_public=0, ctx=None, fmt=FR_MONT):
        """bp_circuit_load_wires: the circuit from what follows the reference's parser.  selectors: QL QR QM QO QC (a dict by column name
        or five arrays; fmt=FR_BYTES_LE: [n, 32] uint8 canonical bytes); wire_ids: [n, 3] uint32 as make_s_polynomials takes them; rows
        0 .. n_public-1 are the public rows.  S1 S2 S3 are built on the GPU.  Selectors given as torch CUDA tensors (int64 [n, 4]) go with
        wire_ids as a CUDA int32 tensor: everything is read in place."""
        self = cls.__new__(cls)
        self.ctx = ctx or default_context()
        sel = [selectors[k] for k in CIRCUIT_COLUMNS[:5]] if isinstance(selectors, dict) else list(selectors)
        on_device = hasattr(wire_ids, "data_ptr")
        if on_device:
            if len(sel) != 5 or not all(hasattr(s, "data_ptr") for s in sel):
                raise BpError(-1, "Circuit.from_wires", "device wire ids go with five device selector columns")
            n = wire_ids.shape[0]
            ok = all(s.shape[0] == n for s in sel) and wire_ids.numel() == 3 * n and wire_ids.element_size() == 4
            ptrs, ids_ptr, keep = [s.data_ptr() for s in sel], wire_ids.data_ptr(), (sel, wire_ids)
        else:
            sel = [_fr_array(s) if fmt == FR_MONT else np.ascontiguousarray(s, dtype=np.uint8).reshape(-1, 32) for s in sel]
            ids = np.ascontiguousarray(wire_ids, dtype=np.uint32)
            n = ids.shape[0]
            ok = len(sel) == 5 and ids.ndim == 2 and ids.shape[1] == 3 and all(len(s) == n for s in sel)
            ptrs, ids_ptr, keep = [s.ctypes.data for s in sel], ids.ctypes.data, (sel, ids)
        if not ok or n < 8 or n & (n - 1):
            raise BpError(-2, "Circuit.from_wires", "five selector columns and [n, 3] wire ids of one power-of-two length >= 8 expected")
        self.group_order, self.n_public = n, n_public
        h = C.c_uint64()
        self.ctx.check(self.ctx._lib.bp_circuit_load_wires(self.ctx._h, n.bit_length() - 1, (C.c_void_p * 5)(*ptrs), ids_ptr, n_public, fmt,
                                                           int(on_device), C.byref(h)), "bp_circuit_load_wires")
        del keep
        self.handle = h.value
        return self

    def load_stats(self):
        """HIP-event milliseconds of the last from_wires on this context, by stage"""
        ms = (C.c_float * 5)()
        self.ctx.check(self.ctx._lib.bp_circuit_load_wires_last_stats(self.ctx._h, ms), "bp_circuit_load_wires_last_stats")
        return dict(zip(("upload_ms", "max_id_ms", "sort_ms", "link_ms", "build_ms"), ms))

    def columns(self, fmt=FR_MONT, names=CIRCUIT_COLUMNS):
        """bp_circuit_export_columns: {column name: [n, 4] Montgomery limbs} of the handle's Lagrange columns (fmt=FR_BYTES_LE: [n, 32]
        uint8); names: the columns wanted"""
        n = self.group_order
        out = {k: (np.zeros((n, 4), dtype=np.uint64) if fmt == FR_MONT else np.zeros((n, 32), dtype=np.uint8)) for k in names}
        ptrs = (C.c_void_p * 8)(*[out[k].ctypes.data if k in out else None for k in CIRCUIT_COLUMNS])
        self.ctx.check(self.ctx._lib.bp_circuit_export_columns(self.ctx._h, self.handle, fmt, ptrs), "bp_circuit_export_columns")
        return out

    def _values(self, values, fmt):
        """a value array as the two assignment calls take it -> (pointer, count, on_device, what to keep alive)"""
        if hasattr(values, "data_ptr"):
            return values.data_ptr(), values.shape[0], 1, values
        v = _fr_array(values) if fmt == FR_MONT else np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 32)
        return v.ctypes.data, len(v), 0, v

    def assign(self, values, fmt=FR_MONT, public_input=True):
        """bp_circuit_assign_device: values[id] per variable ([m, 4] Montgomery limbs, fmt=FR_BYTES_LE: [m, 32] uint8, or a torch CUDA
        tensor int64 [m, 4]) -> Assignment: the columns a, b, c and PI (None with public_input=False) as torch CUDA tensors int64 [n, 4]"""
        import torch
        n = self.group_order
        t = [torch.empty((n, 4), dtype=torch.int64, device=torch.device("cuda", self.ctx.device)) for _ in range(4 if public_input else 3)]
        torch.cuda.synchronize(self.ctx.device)
        ptr, count, on_device, keep = self._values(values, fmt)
        self.ctx.check(self.ctx._lib.bp_circuit_assign_device(self.ctx._h, self.handle, ptr, count, fmt, on_device, t[0].data_ptr(), t[1].data_ptr(),
                                                              t[2].data_ptr(), t[3].data_ptr() if public_input else None), "bp_circuit_assign_device")
        del keep
        return Assignment(t[0], t[1], t[2], t[3] if public_input else None)

    def free(self):
        self.ctx.check(self.ctx._lib.bp_circuit_free(self.ctx._h, self.handle), "bp_circuit_free")

    def commitments(self, setup):
        """Verifier::new (src/verifier.rs:61-68): {column name: 96-byte commitment of its coefficient form}"""
        out = np.zeros(768, dtype=np.uint8)
        self.ctx.check(self.ctx._lib.bp_circuit_commitments(self.ctx._h, setup.handle, self.handle, out.ctypes.data), "bp_circuit_commitments")
        return {k: bytes(out[96 * i: 96 * i + 96]) for i, k in enumerate(CIRCUIT_COLUMNS)}

    def check_sigma(self):
        """bp_circuit_check_sigma: is (S1, S2, S3) a permutation of the cells?  -> SigmaReport; .ok when it is"""
        rep = (C.c_uint64 * 4)()
        self.ctx.check(self.ctx._lib.bp_circuit_check_sigma(self.ctx._h, self.handle, rep), "bp_circuit_check_sigma")
        return SigmaReport(rep[0], _cell(rep[1]), rep[2], _cell(rep[3]))

    def _check(self, ptrs, fmt, on_device):
        rep = (C.c_uint64 * 5)()
        self.ctx.check(self.ctx._lib.bp_circuit_check_witness(self.ctx._h, self.handle, *ptrs, fmt, on_device, rep), "bp_circuit_check_witness")
        return WitnessReport(rep[0], None if rep[1] == _ABSENT else rep[1], rep[2], _cell(rep[3]), _cell(rep[4]))

    def check_witness(self, a, b, c, public_input=None, fmt=FR_MONT):
        """bp_circuit_check_witness: which gate rows and which copy constraints does the witness violate?  a, b, c, public_input as
        Prover.prove_with_blinding takes them (fmt=FR_BYTES_LE: [n, 32] uint8 canonical bytes) -> WitnessReport; .ok when none"""
        n = self.group_order
        if fmt == FR_MONT:
            cols = [_fr_array(v) for v in (a, b, c)] + ([] if public_input is None else [_fr_array(public_input)])
        else:
            cols = [np.ascontiguousarray(v, dtype=np.uint8).reshape(-1, 32) for v in (a, b, c) + (() if public_input is None else (public_input,))]
        if any(len(v) != n for v in cols):
            raise BpError(-6, "check_witness", "witness columns must have group_order entries")
        return self._check([v.ctypes.data for v in cols] + [None] * (4 - len(cols)), fmt, 0)

    def check_witness_device(self, a_ptr, b_ptr, c_ptr, pi_ptr=None, fmt=FR_MONT):
        """same with the witness columns already in HBM (Montgomery limbs), read in place"""
        return self._check([a_ptr, b_ptr, c_ptr, pi_ptr], fmt, 1)

    def check_stats(self):
        """{decode_ms (0: the circuit's decode was cached), upload_ms, check_ms} of the last check on this context"""
        ms = (C.c_float * 3)()
        self.ctx.check(self.ctx._lib.bp_circuit_check_last_stats(self.ctx._h, ms), "bp_circuit_check_last_stats")
        return {"decode_ms": ms[0], "upload_ms": ms[1], "check_ms": ms[2]}


_ABSENT = 0xFFFFFFFFFFFFFFFF


def _cell(v):
    """cell number 3 * row + col of the C ABI -> (col, row); None for an absent position"""
    return None if v == _ABSENT else (int(v) % 3, int(v) // 3)


class Assignment(collections.namedtuple("Assignment", "a b c public_input")):
    """what Circuit.assign returns: the witness columns in HBM (torch CUDA tensors, int64 [n, 4] Montgomery limbs); public_input may
    be None.  Prover.check and Prover.prove_device take them where they are."""
    __slots__ = ()

    def pointers(self):
        return [self.a.data_ptr(), self.b.data_ptr(), self.c.data_ptr(), None if self.public_input is None else self.public_input.data_ptr()]

    def host(self):
        """the columns as [n, 4] uint64 arrays on the host (public_input: None stays None)"""
        return [None if t is None else t.cpu().numpy().view(np.uint64) for t in self]


class SigmaReport(collections.namedtuple("SigmaReport", "bad_labels first_bad_label bad_indegree first_bad_indegree")):
    """counts, and the lowest cell as (col, row), of S values that are no cell label and of cells that are the target of != 1 cells"""
    __slots__ = ()

    @property
    def ok(self):
        return self.bad_labels == 0 and self.bad_indegree == 0


class WitnessReport(collections.namedtuple("WitnessReport", "gate_rows first_gate_row copy_cells first_copy_cell first_copy_target")):
    """rows with a non-zero gate residual (count, lowest row) and cells whose value differs from the value at sigma(cell) (count,
    lowest such cell and its sigma, as (col, row))"""
    __slots__ = ()

    @property
    def ok(self):
        return self.gate_rows == 0 and self.copy_cells == 0


class Prover:
    """src/prover.rs:50-175 behind bp_prove: rounds 1-5 on the GPU, Fiat-Shamir transcript on the host"""

    def __init__(self, setup, circuit):
        assert setup.ctx is circuit.ctx
        self.setup, self.circuit, self.ctx = setup, circuit, setup.ctx

    def prove_with_blinding(self, a, b, c, public_input, blinders):
        """a, b, c: the three Lagrange wire columns (prover.rs:186-227); public_input: the Lagrange column of prover.rs:114-127
        or None; blinders: 11 ints b1..b11 (the reference draws them from thread_rng, prover.rs:108-110).  Returns the 624-byte
        proof: 9 compressed G1 points in Proof field order (verifier.rs:23-40) then the 6 evaluations, 32 bytes LE each."""
        n = self.circuit.group_order
        cols = [_fr_array(v) for v in (a, b, c)]
        pi = None if public_input is None else _fr_array(public_input)
        if any(len(v) != n for v in cols) or (pi is not None and len(pi) != n):
            raise BpError(-6, "prove", "witness columns must have group_order entries")
        bl = np.frombuffer(b"".join((int(v) % Q).to_bytes(32, "little") for v in blinders), dtype=np.uint8).copy()
        if len(bl) != 352:
            raise BpError(-2, "prove", "11 blinders expected")
        out = np.zeros(624, dtype=np.uint8)
        c_ = self.ctx
        c_.check(c_._lib.bp_prove(c_._h, self.setup.handle, self.circuit.handle, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data,
                                  None if pi is None else pi.ctypes.data, FR_MONT, 0, bl.ctypes.data, out.ctypes.data), "bp_prove")
        return bytes(out)

    def prove_device(self, a_ptr, b_ptr, c_ptr, pi_ptr, blinders):
        """same with the witness columns already in HBM (Montgomery limbs)"""
        bl = np.frombuffer(b"".join((int(v) % Q).to_bytes(32, "little") for v in blinders), dtype=np.uint8).copy()
        out = np.zeros(624, dtype=np.uint8)
        c_ = self.ctx
        c_.check(c_._lib.bp_prove(c_._h, self.setup.handle, self.circuit.handle, a_ptr, b_ptr, c_ptr, pi_ptr, FR_MONT, 1, bl.ctypes.data,
                                  out.ctypes.data), "bp_prove")
        return bytes(out)

    def prove_assignment(self, values, blinders, fmt=FR_MONT):
        """bp_prove_assignment on a Circuit.from_wires circuit: values[id] per variable (as Circuit.assign takes them) -> the 624 bytes
        prove_with_blinding returns for the expanded columns"""
        bl = np.frombuffer(b"".join((int(v) % Q).to_bytes(32, "little") for v in blinders), dtype=np.uint8).copy()
        if len(bl) != 352:
            raise BpError(-2, "prove", "11 blinders expected")
        ptr, count, on_device, keep = self.circuit._values(values, fmt)
        out = np.zeros(624, dtype=np.uint8)
        c_ = self.ctx
        c_.check(c_._lib.bp_prove_assignment(c_._h, self.setup.handle, self.circuit.handle, ptr, count, fmt, on_device, bl.ctypes.data,
                                             out.ctypes.data), "bp_prove_assignment")
        del keep
        return bytes(out)

    def check(self, a, b=None, c=None, public_input=None, fmt=FR_MONT):
        """where would prove_with_blinding refuse this witness?  (Circuit.check_witness) -> WitnessReport.  `a` alone may be what
        Circuit.assign returned: the columns are read where they are, in HBM"""
        if isinstance(a, Assignment):
            return self.circuit.check_witness_device(*a.pointers())
        return self.circuit.check_witness(a, b, c, public_input, fmt)

    def last_stats(self):
        r, t = (C.c_float * 5)(), C.c_float()
        self.ctx.check(self.ctx._lib.bp_prove_last_stats(self.ctx._h, r, C.byref(t)), "bp_prove_last_stats")
        return {"round_ms": list(r), "total_ms": t.value}


def make_s_polynomials(wire_ids):
    """Program::make_s_polynomials (src/program.rs:76-147) in O(n log n) on the host (no GPU): wire_ids [n, 3] uint32, 0 = empty
    wire, equal ids = the same variable -> (s1, s2, s3) Lagrange columns as [n, 4] Montgomery limbs"""
    ids = np.ascontiguousarray(wire_ids, dtype=np.uint32)
    n = ids.shape[0]
    if ids.ndim != 2 or ids.shape[1] != 3 or n == 0 or n & (n - 1):
        raise BpError(-2, "make_s_polynomials", "wire_ids must be [2^k, 3]")
    out = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)]
    rc = _lib.load().bp_make_s_polynomials(n.bit_length() - 1, ids.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    if rc:
        raise BpError(rc, "bp_make_s_polynomials", "")
    return tuple(out)


def transcript_test_vector():
    """merlin's conformance vector through the library's host transcript (no GPU needed)"""
    out = np.zeros(32, dtype=np.uint8)
    rc = _lib.load().bp_transcript_test_vector(out.ctypes.data)
    if rc:
        raise BpError(rc, "bp_transcript_test_vector", "")
    return bytes(out)


def _proof_records(proofs):
    """bytes of m x 624, or a list of 624-byte proofs -> (uint8 array, m)"""
    if isinstance(proofs, (list, tuple)):
        proofs = b"".join(bytes(p) for p in proofs)
    rec = proofs if isinstance(proofs, np.ndarray) else np.frombuffer(bytes(proofs), dtype=np.uint8)
    rec = np.ascontiguousarray(rec, dtype=np.uint8).reshape(-1)
    if len(rec) % 624:
        raise BpError(-6, "proofs", "a multiple of 624 bytes expected")
    return rec, len(rec) // 624


def plonk_challenges(proofs, fmt=FR_MONT):
    """Verifier::compute_challengs (verifier.rs:193-209) of m proofs on the host (bp_plonk_challenges, no GPU): [m, 6, 4] uint64
    Montgomery limbs, or [m, 6, 32] canonical little-endian bytes with fmt=FR_BYTES_LE; order beta gamma alpha zeta nu mu.
    An evaluation >= q raises BpError(BP_ERR_BAD_SCALAR) with the record in `index`."""
    rec, m = _proof_records(proofs)
    out = np.zeros((m, 6, 4), dtype=np.uint64) if fmt == FR_MONT else np.zeros((m, 6, 32), dtype=np.uint8)
    bad = C.c_size_t()
    rc = _lib.load().bp_plonk_challenges(rec.ctypes.data if m else None, m, fmt, out.ctypes.data if m else None, C.byref(bad))
    if rc:
        e = BpError(rc, "bp_plonk_challenges", "evaluation >= q in record %d" % bad.value if rc == -4 else "")
        e.index = bad.value if rc == -4 else None
        raise e
    return out


class Verifier:
    """src/verifier.rs:41-79: the verifier's preprocessed input (the eight commitments of Circuit.commitments) for a batch of
    proofs of that circuit.  pairing_inputs returns the two G1 points (A, B) with  batch valid  <=>  pairing(A, x_2) ==
    pairing(B, G2Affine::generator())  (verifier.rs:187-191); verify, verify_each and locate_invalid(decide=None) go on to the
    verdict with the setup's x_2.  Which path computes the pairings is decided by the method called: verify and locate_invalid
    use the host (a batch is two pairings: CPU work), verify_each the GPU (one check per lane)."""

    def __init__(self, setup, circuit):
        assert setup.ctx is circuit.ctx
        self.ctx, self.group_order = setup.ctx, circuit.group_order
        self.x_2 = setup.x_2
        self.commitments = circuit.commitments(setup)
        self.vk = b"".join(self.commitments[k] for k in CIRCUIT_COLUMNS)

    def pairing_inputs(self, proofs, public_inputs, weights=None, challenges=None, fmt=FR_MONT):
        """proofs: m x 624 bytes; public_inputs: [m, n_public] scalars (None: no public inputs); weights: m scalars the caller drew
        after it received the proofs, >= 128 bits of entropy each (None for a single proof)."""
        return self.ctx.verify_reduce(self.group_order.bit_length() - 1, self.vk, proofs, public_inputs, weights, challenges, fmt)

    def pairing_inputs_segments(self, proofs, public_inputs, weights=None, challenges=None, fmt=FR_MONT, segment=1):
        """one pair (A_s, B_s) per segment of `segment` consecutive proofs: pair s is pairing_inputs of that slice alone
        (weights may be None only with segment=1)"""
        return self.ctx.verify_reduce_segments(self.group_order.bit_length() - 1, self.vk, proofs, public_inputs, weights, challenges, fmt, segment)

    def _need_x_2(self, what):
        if self.x_2 is None:
            raise BpError(-1, what, "the setup has no x_2 (pass x_2= to Setup.from_points / from_compressed)")
        return self.x_2

    def verify(self, proofs, public_inputs, weights=None, challenges=None, fmt=FR_MONT):
        """Verifier::verify (verifier.rs:80-192) of the batch, to the end: pairing_inputs, then the pairing check on the host"""
        x_2 = self._need_x_2("Verifier.verify")
        return pairing_check([self.pairing_inputs(proofs, public_inputs, weights, challenges, fmt)], x_2, host=True)[0]

    def verify_each(self, proofs, public_inputs, challenges=None, fmt=FR_MONT):
        """one verdict per proof: one pair per proof (segment = 1, weight 1), then one pairing check per GPU lane"""
        x_2 = self._need_x_2("Verifier.verify_each")
        return pairing_check(self.pairing_inputs_segments(proofs, public_inputs, None, challenges, fmt, 1), x_2, ctx=self.ctx)

    def locate_invalid(self, proofs, public_inputs, weights, decide=None, fmt=FR_MONT):
        """the sorted indices of the proofs of a batch whose own pair fails decide(A96, B96) -> bool, a pairing check
        (pairing(A, x_2) == pairing(B, G2 generator)); decide=None: the host pairing check against the setup's x_2.
        ONE GPU call with segment=1 gives a pair
        per proof; a range's pair is the host sum of its leaves (bp_g1_sum_partials over 144-byte partials), and the search
        descends only into ranges whose sum fails: at most 1 + 2 k ceil(log2 m) decide calls for k bad proofs, 1 for a good batch.
        weights: as pairing_inputs -- they make the sums sound (a failing range may not hide behind cancelling terms)."""
        if decide is None:
            x_2 = self._need_x_2("Verifier.locate_invalid")

            def decide(a96, b96):
                return pairing_check([(a96, b96)], x_2, host=True)[0]
        leaves = self.pairing_inputs_segments(proofs, public_inputs, weights, None, fmt, 1)
        m = len(leaves)
        part_a = b"".join(bytes96_to_partial(a) for a, _ in leaves)
        part_b = b"".join(bytes96_to_partial(b) for _, b in leaves)

        def fails(lo, hi):
            if hi - lo == 1:
                return not decide(*leaves[lo])
            return not decide(sum_partials(part_a[144 * lo: 144 * hi]), sum_partials(part_b[144 * lo: 144 * hi]))
        bad = []
        todo = [(0, m, None)] if m else []                      # (lo, hi, known to fail?)
        while todo:
            lo, hi, known = todo.pop()
            if not (known or fails(lo, hi)):
                continue
            if hi - lo == 1:
                bad.append(lo)
                continue
            mid = (lo + hi + 1) // 2
            # a failing range whose left half passes has its failure on the right: that half needs no decide call of its own
            if fails(lo, mid):
                todo.append((lo, mid, True))
                todo.append((mid, hi, None))
            else:
                todo.append((mid, hi, True))
        return sorted(bad)
