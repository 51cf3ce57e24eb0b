"""-m gpu: multi-GPU behind the C ABI (VERDICT r01 "missing" 1, 2 and 5).

bp_init_multi -- ONE context over a device list: SRS sharded by contiguous point range, MSM / commit / bp_prove fanned out
over the shards and summed, batched host NTTs spread by independent columns.  A 1-GPU box runs it with the device listed
twice or three times (independent shards on one card); with more cards visible the real list is used too.
bp_msm_g1_blob_device / bp_msm_blobs_combine -- the one-process-per-GPU exchange: records stay in HBM, one gather, one D2H.
bp_srs_load_projective144 -- the literal bucket_msm(&[G1Projective], ..) seam."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib
from oracle import oracle as O
from tests import bigint_model as M
from tests import gpu_common as G
from tests import prover_rounds as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = M.Q


def device_lists():
    lists = [[0, 0], [0, 0, 0]]
    if torch.cuda.device_count() >= 2:
        lists.append(list(range(min(torch.cuda.device_count(), 8))))
    return lists


@pytest.fixture(params=[False] + ([True] if G.EXPERIMENT else []), ids=["rehearsal_group"] + (["forced_peer_knob"] if G.EXPERIMENT else []))
def peer(request, monkeypatch):
    """A group that names a device twice ({0, 0}) is a rehearsal group: its members beyond the leader take the GPU-to-GPU branches
    (hipMemcpyPeerAsync behind the leader's event) exactly as members on other cards do -- the lines a multi-GPU node executes run
    here by default (VERDICT r02 next #2a), with no knob.  Experiment build: BP_FORCE_PEER_COPIES=1 also forces the leader's own copies."""
    if request.param:
        monkeypatch.setenv("BP_FORCE_PEER_COPIES", "1")
    return request.param


def test_cpp_single_process_multi_device(tmp_path, peer):
    """the Done-criterion of VERDICT r01 next #2: a single-process C++ program commits through an n-device context and gets
    the single-GPU bytes"""
    exe = str(tmp_path / "test_multi_device")
    libdir = os.path.join(ROOT, "baby_plonk_rust_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "test_multi_device.cpp"), "-o", exe,
                           "-L" + libdir, "-lbp_msm_ntt", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    for devs in device_lists():
        out = subprocess.run([exe, ",".join(map(str, devs))], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "multi device ok (%d shards)" % len(devs) in out.stdout


@pytest.mark.parametrize("devs", device_lists())
def test_group_context_msm_srs_and_tables(devs, peer):
    one, many = bp.Context(0), bp.Context(devs)
    assert many.n_shards() == len(devs) and one.n_shards() == 1
    # the reference's own 1000-point fixture (i * G): load, export, MSM with a closed form
    raw = open(os.path.join(ROOT, "tests", "golden", "g1_uncompressed_valid_test_vectors.dat"), "rb").read()
    h1, hm = one.srs_load(raw), many.srs_load(raw)
    assert many.srs_len(hm) == 1000 and many.srs_export(hm) == raw and many.srs_export(hm, 331, 340) == raw[96 * 331: 96 * 671]
    sc = O.splitmix_scalars(1000, 0xABCD)
    ints = O.fr_array_to_ints(sc)
    want = M.enc96(M.ec_mul(sum(i * s for i, s in enumerate(ints)) % Q))
    assert one.msm(h1, sc) == want and many.msm(hm, sc) == want
    # ranges that start and end inside shards; more scalars than points (zip truncation); device-resident scalars
    for first, cnt in ((0, 1), (333, 1), (332, 3), (100, 777), (999, 5), (1000, 4)):
        w = M.enc96(M.ec_mul(sum((first + i) * s for i, s in enumerate(ints[:min(cnt, 1000 - first)])) % Q))
        assert bp.sum_partials(many.msm_partial(hm, sc[:cnt], first=first)) == w, (first, cnt)
    dsc = torch.from_numpy(sc.view(np.int64)).to("cuda:%d" % devs[0])
    torch.cuda.synchronize()
    assert bp.sum_partials(many.msm_partial(hm, None, first=7, device_ptr=dsc.data_ptr(), n=900)) == \
        M.enc96(M.ec_mul(sum((7 + i) * s for i, s in enumerate(ints[:900])) % Q))
    # canonical-bytes scalars; a value >= q is refused whichever shard meets it
    le = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in ints), dtype=np.uint8).reshape(-1, 32).copy()
    assert many.msm(hm, le, fmt=bp.FR_BYTES_LE) == want
    le[998] = 0xFF
    with pytest.raises(bp.BpError) as e:
        many.msm(hm, le, fmt=bp.FR_BYTES_LE)
    assert e.value.code == -4
    # fixed-base tables on every shard: same bytes, and the table path was taken
    info = many.srs_precompute(hm, 6)
    assert info["window_bits"] == 6 and info["bytes"] == info["windows"] * 1000 * 128
    assert many.msm(hm, sc) == want and many.msm_stats()["tables"]
    many.srs_precompute(hm, bp.SRS_TABLES_OFF)
    assert many.msm(hm, sc) == want and not many.msm_stats()["tables"]
    many.srs_free(hm)
    with pytest.raises(bp.BpError):
        many.srs_len(hm)
    # generated SRSs: every shard produces its own range
    n, tau, a, d = 3001, 0x5EED, 987654321, 1234567
    assert many.srs_export(many.srs_generate(n, tau)) == one.srs_export(one.srs_generate(n, tau))
    hp = many.srs_generate_progression(n, a, d)
    assert many.srs_export(hp, n - 5, 5) == G.progression_bytes(n, a, d)[96 * (n - 5):]
    sc = O.splitmix_scalars(n, 0x77)
    assert many.msm(hp, sc) == M.enc96(M.ec_mul(G.oracle_dot(sc, a, d)))
    # fewer points than shards
    ht = many.srs_generate(1, tau)
    assert many.msm(ht, O.splitmix_scalars(4, 1)) == M.enc96(M.ec_mul(O.fr_array_to_ints(O.splitmix_scalars(4, 1))[0]))
    assert many.msm(many.srs_load(b""), sc) == M.enc96(None)


def test_group_context_msm_2p18_closed_form():
    """a size where every shard runs the full-width pipeline (c = 15 / 16, tables): closed form"""
    many = bp.Context([0, 0])
    n, a, d = 1 << 18, G.Q - 12345, 0x1F2E3D4C5B6A7988
    h = many.srs_generate_progression(n, a, d)
    sc = O.splitmix_scalars(n, 0x5EED0012)
    want = M.enc96(M.ec_mul(O.dot_progression(sc, a, d)))
    assert many.msm(h, sc) == want
    many.srs_precompute(h, 0)
    assert many.msm(h, sc) == want and many.msm_stats()["tables"]


@pytest.mark.parametrize("members", [2, 4])
def test_group_context_round3_by_coset(members, peer, monkeypatch):
    """SURVEY 8e line 3 / VERDICT r02 #5: inside a group context round 3 is split by coset -- each member evaluates a, b, c, z, PI on
    its share of the four cosets s_j <w_n> of the quotient coset, runs the quotient kernel there against its own quarter tables and
    returns n coefficients of t mod (x^n - s_j^n); the leader recombines them with a radix-4 butterfly.  Proof bytes equal the
    single-GPU ones and the same group with the split switched off; with blinders that make the polynomials longer than n (the
    x^(i+n) = s^n x^i fold), a witness that does not satisfy the circuit still fails the same way."""
    from tests.test_gpu_prover_rounds import synthetic_circuit
    one, many = bp.Context(0), bp.Context([0] * members)
    for pn, seed in ((1 << 3, 5), (1 << 7, 6), (1 << 11, 7)):
        cols, pk, public = synthetic_circuit(pn, seed)
        blinders = [random.Random(seed).randrange(1, Q) for _ in range(11)]
        want = None
        for ctx, split, early in ((one, "1", "1"), (many, "1", "1"), (many, "1", "0"), (many, "0", "0")):
            monkeypatch.setenv("BP_PROVE_COSET_SPLIT", split)
            monkeypatch.setenv("BP_PROVE_COSET_EARLY", early)      # a, b, c, PI to the members after round 1 (default) or in round 3
            setup = bp.Setup.generate_srs(pn + 6, 0xC05E7 + pn, ctx)
            circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
            blob = bp.Prover(setup, circuit).prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), None, blinders)
            want = want or blob
            assert blob == want and len(blob) == 624, (pn, members, split, early)
            # an explicit all-zero PI column takes the general path (PI sent, folded and transformed like the others): same bytes
            assert bp.Prover(setup, circuit).prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV([0] * pn), blinders) == want
            if ctx is many and split == "1" and pn == 1 << 7:
                bad = [list(c) for c in cols]
                bad[2][3] = 12345                                         # c no longer equals a * b in row 3
                with pytest.raises(bp.BpError) as e:
                    bp.Prover(setup, circuit).prove_with_blinding(PR.SV(bad[0]), PR.SV(bad[1]), PR.SV(bad[2]), None, blinders)
                assert e.value.code == -11
                # the abandoned proof's early work on the members must not leak into the next one
                assert bp.Prover(setup, circuit).prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), None, blinders) == want
            circuit.free()
    # public inputs through the split (toy circuit of the reference's tests: PI != 0)
    from tests.test_gpu_prover_rounds import toy_circuit
    cols, pk, public = toy_circuit(8)
    blinders = [random.Random(9).randrange(1, Q) for _ in range(11)]
    want = None
    for ctx, early in ((one, "1"), (many, "1"), (many, "0")):
        monkeypatch.setenv("BP_PROVE_COSET_SPLIT", "1")
        monkeypatch.setenv("BP_PROVE_COSET_EARLY", early)
        setup = bp.Setup.generate_srs(8 + 6, 0xABCDE, ctx)
        circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
        blob = bp.Prover(setup, circuit).prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV(public), blinders)
        want = want or blob
        assert blob == want, early
        circuit.free()
    many.close()
    one.close()


def test_group_context_ntt_columns_and_prove(peer):
    from tests.test_gpu_prover_rounds import synthetic_circuit
    one, many = bp.Context(0), bp.Context([0, 0, 0])
    x = np.stack([O.splitmix_scalars(1 << 12, 0xF400 + j) for j in range(7)])
    got = many.ntt_batch(x)
    assert (got == one.ntt_batch(x)).all() and (got[3] == O.ntt_fast(x[3])).all()
    assert (many.ntt_batch(got, inverse=True) == x).all()
    # bp_prove through the group: the nine commitments are sharded, the proof bytes do not change
    pn, tau = 1 << 10, 0x1234567
    cols, pk, public = synthetic_circuit(pn, 11)
    blinders = [random.Random(3).randrange(1, Q) for _ in range(11)]
    blobs = []
    for ctx in (one, many):
        for tables in (False, True):
            setup = bp.Setup.generate_srs(pn + 6, tau, ctx, tables=tables)
            circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
            blobs.append(bp.Prover(setup, circuit).prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), None, blinders))
            assert circuit.commitments(setup) == bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, one).commitments(
                bp.Setup.generate_srs(pn + 6, tau, one, tables=False))
    assert len(blobs[0]) == 624 and all(b == blobs[0] for b in blobs)


@pytest.mark.parametrize("members", [2, 4, 8])
def test_group_context_one_large_transform_default_threshold(members):
    """the shipped library splits ONE host transform over the members from 2^22 elements: same output as one GPU, both directions"""
    one, many = bp.Context(0), bp.Context([0] * members)
    x = O.splitmix_scalars(1 << 22, 0xA122)
    want = one.ntt(x)
    got = many.ntt(x)
    assert (got == want).all() and many.ntt_stats()["members"] == members and one.ntt_stats()["members"] == 1
    assert (many.ntt(got, inverse=True) == x).all()
    small = O.splitmix_scalars(1 << 12, 0xA112)            # below the threshold: the leader alone
    assert (many.ntt(small) == O.ntt_fast(small)).all() and many.ntt_stats()["members"] == 1
    many.close()
    one.close()


@G.experiment
@pytest.mark.parametrize("members", [2, 4, 8])
def test_group_context_one_large_transform(members, monkeypatch):
    """SURVEY 8e, NTT option ii: ONE transform over the members of a group context -- column slices up, pass 1, block exchange,
    remaining passes on slices of e_1, outputs down.  (Members on one card here: the copies between them are device-local.)"""
    monkeypatch.setenv("BP_NTT_GROUP_SPLIT_FROM", "11")
    one, many = bp.Context(0), bp.Context([0] * members)
    for log_n in (11, 12, 13, 16, 19, 20, 21):
        x = O.splitmix_scalars(1 << log_n, 0xA110 + log_n)
        want = O.ntt_fast(x) if log_n <= 16 else one.ntt(x)
        got = many.ntt(x)
        assert (got == want).all(), (members, log_n)
        assert many.ntt_stats()["members"] == (1 if (log_n, members) == (11, 8) else members), (members, log_n)    # 2^11 = 2^6 x 2^5: four column tiles
        assert (many.ntt(got, inverse=True) == x).all(), (members, log_n)
    # canonical little-endian bytes in and out (Scalar::to_bytes), and a shape that does not split (falls back to the leader)
    ints = [random.Random(5).randrange(Q) for _ in range(1 << 12)]
    le = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), dtype=np.uint8).reshape(-1, 32)
    got = many.ntt(le.view(np.uint64).reshape(-1, 4), fmt=bp.FR_BYTES_LE)
    assert (got == one.ntt(le.view(np.uint64).reshape(-1, 4), fmt=bp.FR_BYTES_LE)).all()
    monkeypatch.setenv("BP_NTT_SPLIT", "11:9,2,0")
    x = O.splitmix_scalars(1 << 11, 0xA1FF)
    assert (many.ntt(x) == O.ntt_fast(x)).all()
    assert one.ntt_stats()["members"] == 1
    many.close()
    one.close()


def test_blob_records_one_gather_one_copy():
    """what every rank of the one-process-per-GPU path does, here with three 'ranks' on one card: records written to HBM,
    gathered (a concatenated device tensor stands in for the RCCL all-gather), ONE copy to the host, combined"""
    ctx = bp.Context(0)
    n, a, d = 40000, 424242, 171717
    sc = O.splitmix_scalars(n, 0xD157)
    want = M.enc96(M.ec_mul(G.oracle_dot(sc, a, d)))
    edges = [0, 13000, 13001, 40000]                          # ragged, one single-point shard
    for tables in (False, True):
        gathered = torch.zeros((3, _lib.MSM_BLOB_BYTES), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()          # torch fills on ITS stream; the library writes the record on the context's own
        for r in range(3):
            lo, hi = edges[r], edges[r + 1]
            h = ctx.srs_generate_progression(hi - lo, a + lo * d, d)
            if tables:
                ctx.srs_precompute(h, 0)
            ctx.msm_blob_device(h, gathered[r].data_ptr(), sc[lo:hi])
        assert bp.combine_blobs(gathered.cpu().numpy().tobytes()) == want
    # device-side pre-sum of gathered records (what ShardedMsm does after the all-gather): equal layouts -> one record;
    # different layouts (the ragged shards above pick different window widths) -> marked invalid, the host combines all
    out = torch.zeros(_lib.MSM_BLOB_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.msm_blobs_sum_device(gathered.data_ptr(), 3, out.data_ptr())
    with pytest.raises(bp.BpError):
        bp.combine_blobs(out.cpu().numpy().tobytes())
    for tables in (False, True):
        eq = torch.zeros((4, _lib.MSM_BLOB_BYTES), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for r in range(4):
            h = ctx.srs_generate_progression(10000, a + 10000 * r * d, d)
            if tables:
                ctx.srs_precompute(h, 11)
            ctx.msm_blob_device(h, eq[r].data_ptr(), sc[10000 * r: 10000 * (r + 1)])
        ctx.msm_blobs_sum_device(eq.data_ptr(), 4, out.data_ptr())
        one = out.cpu().numpy().tobytes()
        assert bp.combine_blobs(one) == bp.combine_blobs(eq.cpu().numpy().tobytes()) == want
    # Round 6: a POISONED record among the gathered ones (a rank whose MSM failed before the collective still takes part: header only, its
    # error code and rank; capi_comm.hip) -- here rank 2 of four with BP_ERR_TOO_LARGE.  The device pre-sum carries it into the one record that
    # travels to the host, the host-side combine of all records finds it too, and both report THAT code, never a sum without rank 2's share.
    import struct
    poisoned = eq.clone()
    header = struct.pack("<7Ii2I", 0x424D5042, 0, 0, 0, 0, 0, 0, -10, 2, 0) + bytes(24)        # magic, c, Wr, n_planes, tables, status, entries, err, err_rank, quads, pad
    assert len(header) == 64
    poisoned[2, :64] = torch.frombuffer(bytearray(header), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    ctx.msm_blobs_sum_device(poisoned.data_ptr(), 4, out.data_ptr())
    for blob in (out.cpu().numpy().tobytes(), poisoned.cpu().numpy().tobytes()):
        with pytest.raises(bp.BpError) as e:
            bp.combine_blobs(blob)
        assert e.value.code == -10
    # an empty shard contributes the identity; a corrupt record and a bad scalar are refused
    h = ctx.srs_generate_progression(10, a, d)
    rec = torch.zeros(_lib.MSM_BLOB_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()              # (without this the zero fill can land after the record of an empty shard: seen 19 times in 25)
    ctx.msm_blob_device(h, rec.data_ptr(), sc[:0])
    assert bp.combine_blobs(rec.cpu().numpy().tobytes()) == M.enc96(None)
    with pytest.raises(bp.BpError):
        bp.combine_blobs(bytes(_lib.MSM_BLOB_BYTES))
    bad = np.full((10, 32), 0xFF, dtype=np.uint8)
    ctx.msm_blob_device(h, rec.data_ptr(), bad, fmt=bp.FR_BYTES_LE)
    with pytest.raises(bp.BpError) as e:
        bp.combine_blobs(rec.cpu().numpy().tobytes())
    assert e.value.code == -4


def test_blob_record_is_stream_ordered():
    """ordering against the caller's work is a property of the entry point, not of prose.  With the context on
    the caller's stream (bp_set_stream) the record lands BEHIND a fill the caller enqueued on the destination just before -- no
    synchronize anywhere -- for the enqueue-only form and for the blocking form, for an empty shard (one tiny kernel: round 2 lost
    this race 19 times in 25 on the context's own stream) and for a real one."""
    ctx = bp.Context(0)
    n, a, d = 3000, 97531, 86420
    h = ctx.srs_generate_progression(n, a, d)
    sc = O.splitmix_scalars(n, 0x0DD)
    want = M.enc96(M.ec_mul(G.oracle_dot(sc, a, d)))
    dsc = torch.from_numpy(sc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ctx.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        for trial in range(12):
            for wait in (False, True):
                big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
                big.fill_(0xEE)                                     # ~50 us of fill on the caller's stream, in flight when the call comes
                rec = big[-_lib.MSM_BLOB_BYTES:]
                ctx.msm_blob_device(h, rec.data_ptr(), None, device_ptr=dsc.data_ptr(), n=0, wait=wait)         # empty shard
                assert bp.combine_blobs(rec.cpu().numpy().tobytes()) == M.enc96(None), (trial, wait)
                big.fill_(0x77)
                ctx.msm_blob_device(h, rec.data_ptr(), None, device_ptr=dsc.data_ptr(), n=n, wait=wait)
                out = torch.empty_like(rec)
                out.copy_(rec)                                      # the caller's next operation on the same stream sees the record
                assert bp.combine_blobs(out.cpu().numpy().tobytes()) == want, (trial, wait)
                del big
    st.synchronize()
    ctx.set_stream(None)
    assert ctx.msm(h, sc) == want
    ctx.close()


def test_projective_image_seam():
    """bucket_msm(points: &[G1Projective], ..) (msm.rs:76-81): the points as the reference holds them in memory, z != 1"""
    ctx = bp.Context(0)
    g = O.g1_generator()
    ks = [0, 1, 2, 3, 5, Q - 1, 123456789, 0] + [random.Random(5).randrange(Q) for _ in range(30)]     # identity first, last-but-30 and inside a group
    pts = [O.g1_mul(g, O.fr_from_int(k)) for k in ks]
    assert any(bytes(p.tobytes()[96:144]) != bytes(O.g1_generator().tobytes()[96:144]) for p in pts[2:])      # z != 1: really projective
    h = ctx.srs_load_projective144(b"".join(p.tobytes() for p in pts))
    assert ctx.srs_export(h) == b"".join(M.enc96(M.ec_mul(k)) for k in ks)
    sc = O.splitmix_scalars(len(ks), 3)
    assert ctx.msm(h, sc) == M.enc96(M.ec_mul(sum(k * s for k, s in zip(ks, O.fr_array_to_ints(sc))) % Q))
    # export in the same form (z = 1; identity = (0 : 1 : 0)) and load it back
    img = ctx.srs_export_projective144(h)
    assert bp.sum_partials(img[144 * 4: 144 * 5].tobytes()) == M.enc96(M.ec_mul(5)) and bp.sum_partials(img[:144].tobytes()) == M.enc96(None)
    assert ctx.srs_export(ctx.srs_load_projective144(img)) == ctx.srs_export(h)
    many = bp.Context([0, 0])
    hm = many.srs_load_projective144(b"".join(p.tobytes() for p in pts))
    assert (many.srs_export_projective144(hm) == img).all()
    assert many.srs_export(hm) == ctx.srs_export(h) and many.msm(hm, sc) == ctx.msm(h, sc)


def test_projective_seam_in_one_call(monkeypatch):
    """bp_msm_g1_projective144 = bucket_msm(&[G1Projective], &[Scalar]) with nothing cached: from 2^17 pairs the operands go up in
    pieces (two; BP_SEAM_PIECES) and the multiplication of a piece runs behind the upload of the next.  Same bytes as load + multiply + free and as
    the closed form; the zip truncates to the shorter operand; the small-size and group-context forms are the three calls."""
    ctx = bp.Context(0)
    n, a, d = (1 << 17) + 77, Q - 99991, 0x0F1E2D3C4B5A6978
    h = ctx.srs_generate_progression(n, a, d)
    img = ctx.srs_export_projective144(h)                       # z = 1 images ...
    g = O.g1_generator()
    for at, k in ((0, 0), (5, 7), (n // 2, Q - 2), (n - 1, 0)):  # ... with an identity first and last and two really projective points inside
        img[144 * at: 144 * (at + 1)] = np.frombuffer(O.g1_mul(g, O.fr_from_int(k)).tobytes(), dtype=np.uint8)
    sc = O.splitmix_scalars(n, 0x5EA3)
    ints = O.fr_array_to_ints(sc)
    coef = {0: 0, 5: 7, n // 2: Q - 2, n - 1: 0}
    want = M.enc96(M.ec_mul(sum(s * coef.get(i, (a + i * d) % Q) for i, s in enumerate(ints)) % Q))
    h2 = ctx.srs_load_projective144(img)
    assert ctx.msm(h2, sc) == want
    for pieces in ("1", "2", "3", "4", "0"):                   # "0" is out of range: the default
        monkeypatch.setenv("BP_SEAM_PIECES", pieces)
        assert ctx.msm_projective144(img, sc) == want, pieces
        assert 0 < ctx.msm_stats()["mixed_adds"] <= 64 * n
    monkeypatch.setenv("BP_SEAM_PIECES", "4")                   # the most pieces for the edge cases below
    # fewer scalars than points and fewer points than scalars
    m = n - 12345
    assert ctx.msm_projective144(img, sc[:m]) == ctx.msm(h2, sc[:m])
    assert ctx.msm_projective144(img[: 144 * m], sc) == ctx.msm(h2, sc[:m])
    # canonical bytes; a scalar >= q in the third piece of four is refused, and the next call works as before
    le = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in ints), dtype=np.uint8).reshape(-1, 32).copy()
    assert ctx.msm_projective144(img, le, fmt=bp.FR_BYTES_LE) == want
    le[(5 * n) // 8] = 0xFF
    with pytest.raises(bp.BpError) as e:
        ctx.msm_projective144(img, le, fmt=bp.FR_BYTES_LE)
    assert e.value.code == -4
    assert ctx.msm_projective144(img, sc) == want
    # small sizes and a group context: the three calls underneath
    assert ctx.msm_projective144(img[: 144 * 1000], sc[:1000]) == ctx.msm(h2, sc[:1000])
    assert ctx.msm_projective144(img[:0], sc[:0]) == M.enc96(None)
    many = bp.Context([0, 0])
    assert many.msm_projective144(img, sc) == want
    many.close()
    ctx.close()


def test_group_context_edges():
    """a one-device list is an ordinary context; a bad device id fails like bp_init; records are refused on a group context (it
    combines its own shards); handles of one context mean nothing to another"""
    one = bp.Context([0])
    assert one.n_shards() == 1
    h = one.srs_generate(10, 5)
    ref = bp.Context(0)
    assert one.msm(h, O.splitmix_scalars(10, 1)) == ref.msm(ref.srs_generate(10, 5), O.splitmix_scalars(10, 1))
    with pytest.raises(bp.BpError) as e:
        bp.Context([0, 4096])
    assert e.value.code == -8
    many = bp.Context([0, 0])
    hm = many.srs_generate(100, 7)
    rec = torch.zeros(_lib.MSM_BLOB_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(bp.BpError) as e:
        many.msm_blob_device(hm, rec.data_ptr(), O.splitmix_scalars(100, 2))
    assert e.value.code == -1
    with pytest.raises(bp.BpError):
        one.msm(hm + 1000, O.splitmix_scalars(10, 1))
    # an out-of-range shard offset and an export past the end
    with pytest.raises(bp.BpError):
        many.msm_partial(hm, O.splitmix_scalars(4, 1), first=101)
    with pytest.raises(bp.BpError):
        many.srs_export(hm, 99, 2)
    assert many.srs_export(hm, 100, 0) == b""
    many.close()
    one.close()


def test_commit_many_device():
    """bp_commit_many_device: several Setup::commit calls of one prover round in one call -- same bytes as one at a time, on a
    single-device and on a group context, with polynomials of different lengths (longer than the SRS: zip truncation), an empty one,
    and the Lagrange-basis assertion of setup.rs:34"""
    import time
    for ctx in (bp.Context(0), bp.Context([0, 0, 0])):
        n = 5000
        setup = bp.Setup.generate_srs(n, 0xABCDEF, ctx)
        polys = [bp.DevicePolynomial(O.splitmix_scalars(m, 0xC0 + m), bp.BASIS_MONOMIAL, ctx) for m in (n, n - 6, 0, 17, n + 9, 1)]
        one_by_one = [bp.commit_device(setup, p) for p in polys]
        assert bp.commit_many_device(setup, polys) == one_by_one
        assert one_by_one[2] == M.enc96(None)                         # the empty polynomial: the identity
        assert bp.commit_many_device(setup, polys[:1]) == one_by_one[:1] and bp.commit_many_device(setup, []) == []
        with pytest.raises(bp.BpError):
            bp.commit_many_device(setup, [bp.DevicePolynomial(O.splitmix_scalars(8, 1), bp.BASIS_LAGRANGE, ctx)])
        ctx.close()
    # what it buys at 2^20: three commitments together against three in a row
    ctx = bp.Context(0)
    n = 1 << 20
    setup = bp.Setup.generate_srs(n, 0x1234, ctx)
    t = torch.empty((3, n, 4), dtype=torch.int64, device="cuda")
    for j in range(3):
        ctx.synthetic_scalars_device(t[j].data_ptr(), n, 0x77 + j)
    torch.cuda.synchronize()
    polys = [bp.DevicePolynomial(t[j], bp.BASIS_MONOMIAL, ctx) for j in range(3)]
    want = [bp.commit_device(setup, p) for p in polys]
    assert bp.commit_many_device(setup, polys) == want
    t0 = time.perf_counter()
    for _ in range(3):
        [bp.commit_device(setup, p) for p in polys]
    t1 = time.perf_counter()
    for _ in range(3):
        bp.commit_many_device(setup, polys)
    t2 = time.perf_counter()
    print("three 2^20 commitments: one at a time %.2f ms, together %.2f ms" % (1e3 * (t1 - t0) / 3, 1e3 * (t2 - t1) / 3))
    ctx.close()


def test_srs_ranges_across_shard_seams():
    """every entry point that walks an SRS range over the shards of a group, on ranges that start and end on and around the seams:
    exports in the three encodings are the single-device bytes (and the fixture's), the subgroup check passes shard by shard, the
    tables cover every point once, and a range past the end is refused by each"""
    raw = open(os.path.join(ROOT, "tests", "golden", "g1_uncompressed_valid_test_vectors.dat"), "rb").read()
    raw48 = open(os.path.join(ROOT, "tests", "golden", "g1_compressed_valid_test_vectors.dat"), "rb").read()
    one, many = bp.Context(0), bp.Context([0, 0, 0])
    h1, hm = one.srs_load(raw), many.srs_load(raw)
    n, R = many.srs_len(hm), many.n_shards()
    assert n == 1000 and one.srs_len(h1) == n and R == 3
    # the group's split: contiguous ranges, the first n % R shards one point longer
    seams = [r * (n // R) + min(r, n % R) for r in range(1, R)]
    ranges = [(0, 0), (0, 1), (333, 1), (332, 3), (100, 777), (999, 1), (1000, 0), (0, 1000)]
    for s in seams:                                   # ... and whatever the split is: up to, from and across each seam
        ranges += [(s - 1, 1), (s, 1), (s - 1, 2), (s, 0)]
    assert all(any(f + c == s for f, c in ranges) and any(f == s for f, c in ranges) and any(f < s < f + c for f, c in ranges) for s in seams)
    image = one.srs_export_projective144(h1)
    z = image.reshape(n, 144)[:, 96:]
    identity = np.array([bool(raw[96 * i] & 0x40) for i in range(n)])
    assert identity.any() and not z[identity].any() and z[~identity].any(axis=1).all() and (z[~identity] == z[~identity][0]).all()
    h2 = one.srs_load_projective144(image)            # G1Projective::from(&G1Affine) and back: the image names the fixture's points
    assert one.srs_export(h2) == raw
    for first, cnt in ranges:
        where = (first, cnt)
        assert one.srs_export(h1, first, cnt) == raw[96 * first: 96 * (first + cnt)], where
        assert many.srs_export(hm, first, cnt) == one.srs_export(h1, first, cnt), where
        assert one.srs_export_compressed48(h1, first, cnt) == raw48[48 * first: 48 * (first + cnt)], where
        assert many.srs_export_compressed48(hm, first, cnt) == one.srs_export_compressed48(h1, first, cnt), where
        assert one.srs_export_projective144(h1, first, cnt).tobytes() == image[144 * first: 144 * (first + cnt)].tobytes(), where
        assert many.srs_export_projective144(hm, first, cnt).tobytes() == one.srs_export_projective144(h1, first, cnt).tobytes(), where
        assert many.srs_check_subgroup(hm, first, cnt) is None, where
    for ctx, h in ((one, h1), (many, hm)):
        info = ctx.srs_precompute(h, 6)
        assert info["window_bits"] == 6 and info["windows"] > 0 and info["bytes"] == info["windows"] * 1000 * 128
        assert ctx.srs_table_info(h) == info
    for first, cnt in ((1000, 1), (1001, 0)):
        for ctx, h in ((one, h1), (many, hm)):
            for call in (ctx.srs_export, ctx.srs_export_compressed48, ctx.srs_export_projective144, ctx.srs_check_subgroup):
                with pytest.raises(bp.BpError) as e:
                    call(h, first, cnt)
                assert e.value.code == -1 and "SRS range out of bounds" in str(e.value), (call.__name__, first, cnt)
    many.close()
    one.close()
