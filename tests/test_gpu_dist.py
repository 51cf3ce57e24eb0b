"""-m gpu: the N > 1 path with real GPU partials: two ranks (gloo, both on GPU 0 -- this box has one card), each holding a
point-range shard of the SRS in HBM, all-gather of the 144-byte partials, host combine.  Also rehearses bench.py's N = 2
control flow end to end (barriers, max-over-ranks timing, rank-0 JSON line)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import baby_plonk_rust_amd as bp
        from baby_plonk_rust_amd import dist as bpd
        from oracle import oracle as O
        ctx = bp.Context(0)
        a, d = 424242, 171717
        lo, hi = bpd.shard_range(n, rank, world)
        srs = ctx.srs_generate_progression(hi - lo, a + lo * d, d)            # this rank's point range, resident in HBM
        sc = O.splitmix_scalars(n, 0xD157)[lo:hi]
        q.put((rank, bpd.msm_sharded(ctx, srs, sc)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_point_range_shards_on_one_gpu():
    from oracle import oracle as O
    from tests import bigint_model as M
    world, n = 2, 5000
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = M.enc96(M.ec_mul(O.dot_progression(O.splitmix_scalars(n, 0xD157), 424242, 171717)))
    assert all(got == want for _, got in res)


def test_bench_self_launches_two_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the parent starts the two ranks itself (before touching the GPU) and
    relays rank 0's line.  gloo backend = a rehearsal of the N > 1 control flow on a 1-GPU box: barriers, max-over-ranks timing,
    the records' all-gather, both scaling legs, the rank-0 JSON line."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--log-n", "14", "--ntt-log-n", "14",
           "--strong-log-n", "15", "--prove-log-n", "10", "--prove-reps", "2", "--backend", "gloo", "--skip-cpu", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    # under a launcher rank 0 prints a COMPLETE line after the weak leg and after every later leg, each relayed as it arrives: a kill
    # in a later leg leaves the newest finished line in the caller's tail (VERDICT r05 #1c)
    assert len(lines) >= 2 and all(l["provisional"] for l in lines[:-1]) and lines[-1]["provisional"] is False
    assert lines[0]["legs_finished"] == ["weak_msm"] and lines[0]["value"] > 0 and lines[0]["n_gpus"] == 2 and "roofline" in lines[0]
    assert all(a["legs_finished"] == b["legs_finished"][:len(a["legs_finished"])] and len(b["legs_finished"]) == len(a["legs_finished"]) + 1
               for a, b in zip(lines, lines[1:-1]))
    assert lines[-1]["legs_finished"] == ["weak_msm", "ntt", "ntt_columns", "strong_msm", "group_commit", "prove", "one_proof_over_all_gpus"]
    assert all(l["value"] == lines[0]["value"] and l["ms_per_step"] == lines[0]["ms_per_step"] for l in lines)      # the headline does not move between lines
    line = lines[-1]
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0 and line["ntt"]["value"] > 0
    assert line["config"]["msm_points_per_gpu"] == 1 << 14 and len(line["per_rank"]) == 2
    st = line["strong_scaling"]
    assert st["scaling"] == "strong" and st["n_gpus"] == 2 and st["points_per_rank"] == 1 << 14 and st["value"] > 0
    assert len(st["accumulate_ms_per_rank"]) == 2 and all(v > 0 for v in st["accumulate_ms_per_rank"])
    assert line["prove"]["gates"] == 1 << 10 and line["prove"]["value"] > 0 and line["prove"]["parallelism"] == "independent proofs x2"
    cols = line["ntt_columns"]                              # the NTT half of the N > 1 contract: columns over the ranks + ONE all-gather
    assert cols["n_gpus"] == 2 and cols["columns"] == 23 and cols["columns_per_rank"] == [12, 11] and cols["value"] > 0
    assert cols["foreign_column_matches_local_transform"] is True and cols["same_on_all_ranks"] is True and cols["allgather_ms_per_step"] > 0
    gc = line["group_commit"]                               # the bp_init_multi seam beside the ranks: peer matrix + per-member split in the line
    assert gc.get("same_result") is True and len(gc["per_member"]) == 2 and gc["peer_access"]["devices"] == [0, 0], gc
    grp = line["prove"]["one_proof_over_all_gpus"]          # one proof on a context spanning all ranks' GPUs (here: two shards on one card)
    assert len(grp["last_commit_per_member"]) == 2 and "can_access_peer" in grp["peer_access"], grp
    assert grp["n_gpus"] == 2 and grp.get("same_proof_bytes_as_one_gpu") is True and grp["latency_ms_per_proof"] > 0, grp
    # the strong-scaling problem is the same for every N: one rank must get the same bytes
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--log-n", "14", "--ntt-log-n", "14",
                          "--strong-log-n", "15", "--prove-log-n", "0", "--skip-cpu", "--skip-seams", "--other-sizes", "--full"], capture_output=True, text=True,
                         timeout=900, cwd=ROOT, env=env)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    line1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert line1["n_gpus"] == 1 and line1["strong_scaling"]["result_sha"] == st["result_sha"]


def test_bench_keeps_the_finished_legs_when_a_rank_stops_taking_part():
    """VERDICT r05 #1c: the first N > 1 run must not be losable.  Rehearsal (gloo, two ranks on this card): rank 1 stops after the NTT leg;
    rank 0 runs into the next collective and stays there; the watchdog ends the ranks after --leg-timeout, the parent exits non-zero --
    and the COMPLETE lines of the legs that did finish (weak MSM, NTT) have been relayed and are what the caller keeps."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--log-n", "14", "--ntt-log-n", "14",
           "--strong-log-n", "15", "--prove-log-n", "0", "--backend", "gloo", "--skip-cpu", "--skip-group-legs", "--leg-timeout", "25", "--full",
           "--rehearse-hang-after", "ntt"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode != 0, out.stdout[-1000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [l["legs_finished"] for l in lines] == [["weak_msm"], ["weak_msm", "ntt"]] and all(l["provisional"] for l in lines), out.stdout[-2000:]
    assert lines[-1]["value"] > 0 and lines[-1]["n_gpus"] == 2 and lines[-1]["ntt"]["value"] > 0 and "roofline" in lines[-1]
    assert "giving up" in out.stderr and "'ntt'" in out.stderr, out.stderr[-2000:]


def test_bench_refuses_more_ranks_than_gpus():
    import torch
    n = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1), "--steps", "1", "--warmup", "0"], capture_output=True,
                         text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 2 and "--gpus %d" % (n + 1) in out.stderr and not out.stdout.strip()


def test_bench_under_launcher_with_rccl_single_rank():
    """one rank under torch.distributed.run with the RCCL backend: the exchange path of N > 1 (records all-gathered on the device by
    RCCL, one D2H, combine; gloo side group for host gathers) really runs, with a world of one -- what a 1-GPU box can execute"""
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--log-n", "16", "--ntt-log-n", "16", "--strong-log-n", "17",
           "--prove-log-n", "0", "--skip-cpu", "--skip-seams", "--other-sizes", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["config"]["backend"] == "nccl" and line["strong_scaling"]["rccl_ranks"] == 1
    assert line["exchange_ms"] > 0 and line["strong_scaling"]["exchange_ms_per_rank"][0] > 0
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    one = subprocess.run([sys.executable] + cmd[10:], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    line1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert line1["result_sha"] == line["result_sha"] and line1["strong_scaling"]["result_sha"] == line["strong_scaling"]["result_sha"]
    assert line1["config"]["backend"] is None


def _comm_worker(q):
    try:
        _comm_body(q)
    except BaseException:
        import traceback
        q.put(traceback.format_exc())
        raise


def _comm_body(q):
    """RCCL through the C ABI only (no torch.distributed): what a Rust host that runs one process per GPU binds"""
    import numpy as np
    import torch

    import baby_plonk_rust_amd as bp
    from oracle import oracle as O
    from tests import bigint_model as M
    ctx = bp.Context(0)
    assert ctx.comm_info() == (0, 0)
    n, a, d = (1 << 16) + 77, 31337, 271828
    h = ctx.srs_generate_progression(n, a, d)
    ctx.srs_precompute(h)
    sc = O.splitmix_scalars(n, 0xC0BB)
    want = M.enc96(M.ec_mul(O.dot_progression(sc, a, d)))
    try:
        ctx.msm_allgather(h, sc)
        q.put("no communicator must be an error")
        return
    except bp.BpError as e:
        assert e.code == -1
    ctx.comm_init_rank(bp.Context.comm_unique_id(), 0, 1)             # rank 0 of a world of one: ncclGetUniqueId + ncclCommInitRank
    assert ctx.comm_info() == (0, 1)
    got = ctx.msm_allgather(h, sc)                                    # record -> ncclAllGather -> device pre-sum -> one D2H -> combine
    assert got == want == ctx.msm(h, sc), "bp_msm_g1_allgather differs from bp_msm_g1"
    assert ctx.comm_last_exchange_ms() > 0
    t = torch.from_numpy(sc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert ctx.msm_allgather(h, None, device_ptr=t.data_ptr(), n=n) == want
    assert ctx.msm_allgather(h, sc[:1000], first=500) == M.enc96(M.ec_mul(O.dot_progression(sc[:1000], a + 500 * d, d)))
    assert ctx.msm_allgather(h, sc[:0]) == M.enc96(None)             # an empty range still takes part in the collective
    bad = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in (1, M.Q, 2)), dtype=np.uint8).reshape(-1, 32)
    try:
        ctx.msm_allgather(h, bad, fmt=bp.FR_BYTES_LE)
        q.put("scalar >= q must be rejected")
        return
    except bp.BpError as e:
        assert e.code == -4
    # NTT columns: 3 columns of 2^12 in this rank's (only) block; the in-place all-gather of a world of one leaves them as they are
    cols = O.splitmix_scalars(3 << 12, 0xC01).reshape(3, 1 << 12, 4)
    tc = torch.from_numpy(cols.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    for j in range(3):
        ctx.ntt_device(tc[j].data_ptr(), 12)
    ctx.ntt_columns_allgather(tc.data_ptr(), 12, 3)
    out = tc.cpu().numpy().view(np.uint64)
    assert all((out[j] == O.ntt_fast(cols[j])).all() for j in range(3))
    try:
        ctx.comm_init_rank(bp.Context.comm_unique_id(), 0, 1)
        q.put("a second communicator on one context must be an error")
        return
    except bp.BpError as e:
        assert e.code == -1
    # VERDICT r05 #1a: a rank NEVER skips a collective.  A local failure in front of the all-gather (here: `first` beyond the shard, an
    # unknown handle) still enqueues it -- the collective counter advances -- and comes back as that error; the communicator stays usable
    assert ctx.comm_stats()["timeout_ms"] == 120000
    for kwargs, code, text in (({"first": n + 1}, -1, "out of bounds"), ({"handle": h + 12345}, -1, "")):
        before = ctx.comm_stats()["collectives"]
        try:
            ctx.msm_allgather(kwargs.get("handle", h), sc[:100], first=kwargs.get("first", 0))
            q.put("a local failure in front of the collective must still be an error: %r" % (kwargs,))
            return
        except bp.BpError as e:
            assert e.code == code and text in str(e), str(e)
        assert ctx.comm_stats()["collectives"] == before + 1, "the failing rank stayed away from the all-gather"
        assert ctx.comm_info() == (0, 1) and ctx.msm_allgather(h, sc) == want
    before = ctx.comm_stats()["collectives"]
    try:
        ctx.ntt_columns_allgather(tc.data_ptr(), 29, 3)               # bad shape: said INSIDE the agreement all-gather, no column moves
        q.put("columns longer than 2^28 must be an error")
        return
    except bp.BpError as e:
        assert e.code == -10
    assert ctx.comm_stats()["collectives"] == before + 1
    ctx.ntt_columns_allgather(tc.data_ptr(), 12, 3)
    assert ctx.comm_stats()["collectives"] == before + 3              # agreement + the columns
    # VERDICT r05 #1b: every wait behind a collective is bounded.  A 1-ms bound under a 2^21-point table-free MSM (~7 ms of kernels in front
    # of the all-gather): BP_ERR_COMM, the communicator aborted -- not a stall; a new communicator works afterwards
    big = ctx.srs_generate_progression(1 << 21, a, d)
    sc_big = O.splitmix_scalars(1 << 21, 0xB16)
    want_big = M.enc96(M.ec_mul(O.dot_progression(sc_big, a, d)))
    assert ctx.msm_allgather(big, sc_big) == want_big                 # (first call at this size: workspaces grow, which waits for the stream inside the launch)
    ctx.comm_set_timeout_ms(1)
    try:
        ctx.msm_allgather(big, sc_big)
        q.put("a 1-ms bound must expire under a 7-ms pipeline")
        return
    except bp.BpError as e:
        assert e.code == -12 and "did not finish within 1 ms" in str(e), str(e)
    assert ctx.comm_info() == (0, 0)
    ctx.synchronize()
    ctx.comm_set_timeout_ms(120000)
    ctx.comm_init_rank(bp.Context.comm_unique_id(), 0, 1)
    assert ctx.msm_allgather(big, sc_big) == want_big
    ctx.comm_destroy()
    assert ctx.comm_info() == (0, 0)
    ctx.comm_init_rank(bp.Context.comm_unique_id(), 0, 1)             # and again after a destroy
    assert ctx.msm_allgather(h, sc) == want
    ctx.close()                                                       # bp_destroy releases the communicator
    q.put("ok")


def test_rccl_collectives_under_the_c_abi_world_of_one():
    """the all-gather of the MSM records and of finished NTT columns is reachable through the C ABI alone
    (bp_comm_unique_id / bp_comm_init_rank / bp_msm_g1_allgather / bp_ntt_columns_allgather; libbp_msm_ntt.so links librccl).
    A world of one rank is what a one-GPU box can run: same bytes as bp_msm_g1, errors as errors."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_comm_worker, args=(q,))
    p.start()
    res = q.get(timeout=600)
    p.join(timeout=120)
    assert res == "ok" and p.exitcode == 0, res


def _missing_rank_worker(q):
    import time
    import baby_plonk_rust_amd as bp
    try:
        ctx = bp.Context(0)
        ctx.comm_set_timeout_ms(500)
        t0 = time.perf_counter()
        try:
            ctx.comm_init_rank(bp.Context.comm_unique_id(), 0, 2)      # a world of two whose rank 1 never calls: ncclCommInitRank would block for ever
            q.put("an init without its second rank must not succeed")
        except bp.BpError as e:
            waited = time.perf_counter() - t0
            assert e.code == -12 and "did not return within 500 ms" in str(e), str(e)
            assert 0.4 < waited < 30, waited
            assert ctx.comm_info() == (0, 0)
            try:
                ctx.comm_init_rank(bp.Context.comm_unique_id(), 0, 1)  # the helper thread is still inside RCCL: this context takes no further communicator
                q.put("a context whose init is stuck must refuse another")
            except bp.BpError as e2:
                assert e2.code == -12 and "still inside RCCL" in str(e2)
                other = bp.Context(0)                                  # a fresh context of the same process is fine
                other.comm_init_rank(bp.Context.comm_unique_id(), 0, 1)
                assert other.comm_info() == (0, 1)
                q.put("ok")
    except BaseException:
        import traceback
        q.put(traceback.format_exc())
    finally:
        q.close()
        q.join_thread()        # the answer is on its way to the parent (Queue.put only hands it to a feeder thread) ...
        os._exit(0)            # ... before this: the parked helper thread sits in RCCL's bootstrap, so leave without running RCCL's static destructors


def test_comm_init_is_bounded_when_a_rank_never_arrives():
    """VERDICT r05 #1b: ncclCommInitRank blocks until every rank of the world has called it; with a bound it is BP_ERR_COMM instead of a
    stall (the reference panics, it never blocks: src/setup.rs:34)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_missing_rank_worker, args=(q,))
    p.start()
    try:
        res = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert res == "ok", res
