"""The multi-device paths: the thread-group communicator with hipMemcpyPeerAsync between two devices, the
RCCL communicator of world 2 across two devices (its all-gather, its grouped send/recv, one rb3gpu_sh_merge through it), the
shard object over two devices, and the CLI's `build --gpus 2` / `--gpus 2 --interval` with distinct devices.  Rank r runs on
device r % (devices of the box): on a one-GPU box the ranks share device 0 and every test but the RCCL one runs the same calls
with the copies between ranks staying on that device; RCCL refuses two ranks on one device, so that test needs two.  No
multi-GPU box was available in rounds 1-5: until one is, the copies between distinct devices are UNMEASURED on hardware."""
import hashlib
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from ropebwt3_amd import _build
from tests import util
from tests.test_gpu_engine import _sharded_case, _check_interval

pytestmark = pytest.mark.gpu


def _ndev():
    try:
        from ropebwt3_amd import gpu
        return int(gpu.load_library().rb3gpu_device_count())
    except Exception:
        return 0


NDEV = _ndev()
need2 = pytest.mark.skipif(NDEV < 2, reason="needs two HIP devices (this box has %d)" % NDEV)
MAN = json.load(open(os.path.join(util.GOLDEN, "MANIFEST.json")))


@pytest.mark.parametrize("world", [2, min(4, max(NDEV, 2))])
def test_thread_group_communicator_over_distinct_devices(oracle, world):
    """rb3gpu_sh_merge with one rank per DEVICE: the thread-group communicator's all-to-all is hipMemcpyPeerAsync between two
    devices here (every rank pulls its share), its barriers join threads that drive different devices (one device: the ranks share it)"""
    from ropebwt3_amd import Rb3Gpu, CommGroup, multi
    rng = np.random.default_rng(700 + world)
    cur, batches, want = _sharded_case(oracle, rng, "reads")
    bounds0 = multi.interval_bounds(cur.size, world)
    grp = CommGroup(world)
    errs = []

    def run(rank):
        try:
            r = np.random.default_rng(900 + rank)
            h = Rb3Gpu(device=rank % NDEV, verbose=1)
            assert h._lib.rb3gpu_device_of(h._h) == rank % NDEV
            comm = grp.comm(rank, h)
            bounds = bounds0
            h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
            for b, t2 in enumerate(batches):
                d_bwt, d_tw = h.sort_text(t2)
                bounds, _ = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0), commit=True)
                h.dev_free(d_bwt), h.dev_free(d_tw)
                _check_interval(h, r, want[b + 1], bounds, rank)
            h.close()
        except BaseException as e:
            errs.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    grp.close()
    assert not errs, errs


def test_shard_object_over_two_devices(oracle):
    """rb3gpu_shard_split / _merge / _gather with the intervals on devices 0 and 1 (what `build --gpus 2 --interval` calls; one device: both on it)"""
    from ropebwt3_amd import Rb3Gpu, Shard
    rng = np.random.default_rng(41)
    cur, batches, want = _sharded_case(oracle, rng, "family")
    h = Rb3Gpu(verbose=1)
    try:
        h.from_plain(cur)
        sh = Shard(h, [0, 1 % NDEV])
        for t2 in batches:
            d_bwt, d_tw = h.sort_text(t2)
            sh.merge(d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            h.dev_free(d_bwt), h.dev_free(d_tw)
        sh.gather()
        assert np.array_equal(h.export_plain(), want[-1])
    finally:
        h.close()


def _rccl_worker(rank, world, uid, q):
    try:
        import ctypes
        from ropebwt3_amd import Rb3Gpu, RcclComm, gpu, multi
        from tests.util import Oracle
        oracle = Oracle()
        cur, batches, want = _sharded_case(oracle, np.random.default_rng(77), "reads")   # (same seed: every rank makes the same case)
        h = Rb3Gpu(device=rank, verbose=1)
        comm = RcclComm(h, rank, world, uid)
        # all-gather of a vector of 64-bit counts
        ag = gpu.ALL_GATHER_F(comm.struct.all_gather)
        send, recv = (ctypes.c_int64 * 3)(rank, 10 * rank, 7), (ctypes.c_int64 * (3 * world))()
        assert ag(comm.struct.ctx, send, 3, recv) == 0
        assert list(recv) == [v for r in range(world) for v in (r, 10 * r, 7)]
        # grouped send/recv: rank r sends 100 * (p + 1) states of 16 bytes to rank p, tagged with sender and receiver
        a2a = gpu.ALL_TO_ALL_F(comm.struct.all_to_all)
        cap = 100 * world
        stride = cap
        st = np.zeros((world, stride, 2), dtype=np.int64)
        for p in range(world):
            st[p, :100 * (p + 1), 0] = rank
            st[p, :100 * (p + 1), 1] = p * 1000 + np.arange(100 * (p + 1))
        d_s, d_r = h.dev_alloc(st.nbytes), h.dev_alloc(st.nbytes)
        h.dev_upload_to(d_s, st)
        scnt = (ctypes.c_int64 * world)(*[100 * (p + 1) for p in range(world)])
        rcnt = (ctypes.c_int64 * world)(*[100 * (rank + 1)] * world)
        assert a2a(comm.struct.ctx, d_s, stride, scnt, d_r, rcnt, h._lib.rb3gpu_stream_of(h._h)) == 0
        h.sync()
        got = h.dev_download_i64(d_r, 2 * 100 * (rank + 1) * world).reshape(world, 100 * (rank + 1), 2)
        for p in range(world):
            assert np.all(got[p, :, 0] == p) and np.array_equal(got[p, :, 1], rank * 1000 + np.arange(100 * (rank + 1)))
        h.dev_free(d_s), h.dev_free(d_r)
        # one interval-sharded merge per batch through it
        bounds = multi.interval_bounds(cur.size, world)
        h.from_plain(cur[bounds[rank]:bounds[rank + 1]])
        for b, t2 in enumerate(batches):
            d_bwt, d_tw = h.sort_text(t2)
            bounds, _ = h.sh_merge(comm, bounds, d_bwt, d_tw, t2.size, np.flatnonzero(t2 == 0))
            h.dev_free(d_bwt), h.dev_free(d_tw)
            _check_interval(h, np.random.default_rng(rank), want[b + 1], bounds, rank)
        comm.close()
        h.close()
        q.put((rank, True, ""))
    except BaseException as e:
        import traceback
        q.put((rank, False, traceback.format_exc()[-1500:] + repr(e)))


@need2
def test_rccl_communicator_world_two_across_two_devices():
    """one PROCESS per device, joined by RCCL over xGMI (librccl loaded by the library): all-gather, grouped send/recv with uneven
    counts, and rb3gpu_sh_merge of three batches through it -- the intervals are the oracle's after every batch"""
    import multiprocessing as mp
    from ropebwt3_amd import RcclComm
    uid = RcclComm.unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 2
    env = dict(os.environ)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        procs = [ctx.Process(target=_rccl_worker, args=(r, world, uid, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = sorted(q.get(timeout=900) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.clear(), os.environ.update(env)
    assert all(r[1] for r in res), res


def _cli(args):
    r = subprocess.run([_build.BIN_CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    return r.stdout, r.stderr.decode()


@pytest.mark.parametrize("mode", [[], ["--interval"]])
def test_cli_build_on_two_devices(mode):
    """`build --gpus 2` (slices + tree merge, peer copy of the right operand) and `build --gpus 2 --interval` with the two
    handles on DIFFERENT devices (one device: both handles on it): the reference's .fmd"""
    for name, extra in (("reads_fwd", ["-m40k"]), ("reads_fq", ["-m40k"]), ("genomes12_files", [])):
        if mode and name == "genomes12_files":
            continue   # (--interval is for batches of short strings)
        ent = MAN[name]
        inputs = [os.path.join(util.GOLDEN, p) for p in ent["inputs"]]
        out, err = _cli(["build"] + ent.get("flags", []) + ["-d", "--gpus", "2"] + mode + extra + inputs)
        assert hashlib.md5(out).hexdigest() == ent["fmd_md5"], (name, mode)


def test_this_file_reports_the_device_count():
    """(always runs: the log of a GPU run says how many devices the multi-device tests saw)"""
    print("HIP devices visible: %d -- ranks of the multi-device tests %s" % (NDEV, "on distinct devices" if NDEV >= 2 else "share device 0; the RCCL test skipped"))
    assert NDEV >= 1
