"""Multi-part device path: N processes (one part each, RCCL ghost exchange inside libpamg,
gloo for the host setup) must reproduce the global-view oracle's multi-part V-cycle bit for
bit (SPEC §S7: the operators are the global ones, only their storage is partitioned).

On a one-GPU box all ranks share device 0 (RCCL permitting); the driver's 8-GPU node runs
the same code one rank per device."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _collect(procs, q, timeout):
    """Each rank's result; fails fast (instead of waiting out the timeout) when a rank died
    without reporting — the others would block in a collective for ever."""
    import queue
    import time
    res, t0 = {}, time.time()
    while len(res) < len(procs):
        try:
            r = q.get(timeout=5)
            res[r[0]] = r
            continue
        except queue.Empty:
            pass
        dead = [i for i, p in enumerate(procs) if p.exitcode not in (None, 0) and i not in res]
        if dead or time.time() - t0 > timeout:
            for p in procs:
                if p.is_alive():
                    p.kill()
            raise AssertionError(f"ranks {dead} died (exit codes {[procs[i].exitcode for i in dead]})" if dead
                                 else f"no result within {timeout} s")
    for p in procs:
        p.join(timeout=60)
    return res


def _worker(rank, world, port, kind, n, max_coarse, agglomerate, ncycles, poison, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), OMP_NUM_THREADS="2")
    import ctypes

    import parallel_amg_amd as pa
    from parallel_amg_amd import _lib
    from parallel_amg_amd._lib import call
    from parallel_amg_amd.partitioned import Context, PVector, mul
    from parallel_amg_amd.solver import AMGSolver
    _lib.lib()  # before torch: /opt/rocm's HIP/RCCL (see _lib.runtime_providers)
    import torch.distributed as dist
    try:
        # SURVEY §5 race check: ghosts are NaN until their exchange lands
        call("pamg_set_option", b"poison_ghosts", int(poison))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        be = pa.DistributedBackend()
        if kind.startswith("mtx:"):
            A, offs, xs = pa.load_problem(be, kind[4:])
        elif kind.startswith("rcm:"):  # rcm:<kind>: shuffled, then the graph partitioner
            whole, _o, wx = pa.generate_problem(pa.SequentialBackend(1), kind[4:], n)
            whole, wx = pa.permute_problem(whole, wx, 11)
            whole, wx, _perm = pa.rcm_problem(whole, wx)
            A, offs, xs = pa.split_problem(be, whole, wx, "nnz")
        else:
            A, offs, xs = pa.generate_problem(be, kind, n)
        H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=max_coarse, agglomerate=agglomerate))
        nd = ctypes.c_int()
        call("pamg_device_count", ctypes.byref(nd))
        ndev = max(1, nd.value)
        # RCCL needs one device per rank; with fewer GPUs than ranks use the host transport
        ctx = Context(rank % ndev, be, transport="rccl" if ndev >= world else "host")
        S = AMGSolver(ctx, H, part=rank)
        A0 = S.A[0]
        xst = PVector(ctx, A0.n_own_cols, A0.n_ghost, xs[rank])
        b = PVector(ctx, A0.nrows)
        mul(b, A0, xst)
        x = S.new_vector()
        hist = S.vcycle(x, b, ncycles, res_hist=True)
        # the same cycles as one stationary run: the cross-cycle pipeline where the parts qualify
        # (z-slabs of whole planes), separate cycles otherwise — the same bits either way
        xp = S.new_vector()
        S.vcycle(xp, b, ncycles)
        same_pipe = bool(np.array_equal(xp.own_values().view(np.int64), x.own_values().view(np.int64)))
        # consistent!(x) split (exchange_begin/_end) == the synchronous exchange == the
        # owners' values at the ghost ids
        ghosts = None
        pl = H.levels[0][rank].planA
        if S.A[0].plan is not None:
            from parallel_amg_amd.partitioned import consistent, consistent_async
            va = PVector(ctx, pl.n_own, pl.n_ghost, x.own_values())
            vb = PVector(ctx, pl.n_own, pl.n_ghost, x.own_values())
            consistent(va, S.A[0].plan)
            consistent_async(vb, S.A[0].plan).wait()
            ga, gb = va.ghost_values(), vb.ghost_values()
            assert np.array_equal(ga.view(np.int64), gb.view(np.int64))
            ghosts = (np.asarray(pl.ghost_ids, np.int64), ga)
        out = (rank, "ok", b.own_values(), x.own_values(), hist, ghosts, _lib.layout_of(S.A[0])["jr_fused"], same_pipe)
        q.put(out)
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None, None, None, None, None, None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world,kind,n,max_coarse,agglomerate,poison", [
    (2, "poisson3d", 20, 100, 0, 1),       # decoupled on every level, coarsest gathered
    (2, "poisson3d", 20, 100, 32768, 0),   # agglomerated from level 1 on (SPEC §S7)
    (3, "poisson2d", 60, 200, 0, 1),
    (3, "aniso3d", 16, 30, 600, 1),        # agglomerated from level 2 on
    (2, "poisson2d", 20, 1000, 0, 0),      # one level: the distributed coarsest solve
    (3, "poisson2d", 36, 2000, 0, 1),      # one level of 1,296 rows: row offsets != 0, a second 1,024-column chunk
    (4, "poisson3d", 24, 60, 0, 1),        # four parts, interior parts with two neighbours
    # eight parts (BASELINE.json configs[2]'s part count) at a size the oracle sets up in
    # seconds: decoupled on every level and agglomerated (SPEC §S7)
    (8, "poisson3d", 64, 1000, 0, 1),
    (8, "poisson3d", 64, 1000, 32768, 0),
    (8, "aniso3d", 64, 1000, 0, 1),
    (8, "aniso3d", 64, 1000, 32768, 1),
])
def test_multipart_vcycle_bit_exact(world, kind, n, max_coarse, agglomerate, poison, built):
    from oracle import oracle as O
    ncycles = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, kind, n, max_coarse, agglomerate, ncycles, poison, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, 600)
    for r in range(world):
        assert res[r][1] == "ok", res[r][1]
    Ao = O.generate(kind, *O.grid_shape(kind, n))
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    Ho = O.setup(Ao, nparts=world, max_coarse=max_coarse, agglomerate=agglomerate)
    xo, ho = Ho.solve(bo, ncycles, res_hist=True)
    if kind == "poisson2d" and n * n <= max_coarse:
        assert Ho.nlevels == 1   # (the dense solve of the ranks' own rows is the whole cycle)
    b = np.concatenate([res[r][2] for r in range(world)])
    x = np.concatenate([res[r][3] for r in range(world)])
    bits = lambda a: np.asarray(a, np.float64).view(np.int64)
    assert np.array_equal(bits(b), bits(bo))
    assert np.array_equal(bits(x), bits(xo))
    if n == 64 and kind in ("poisson3d", "aniso3d"):
        # every part is a z-slab of whole planes: the level-0 Jacobi -> residual runs as the
        # blocked pass on the slab's inner planes (SymDia::tb_part) — the bits above are its
        assert all(res[r][6] for r in range(world)), [res[r][6] for r in range(world)]
    assert all(res[r][7] for r in range(world)), [res[r][7] for r in range(world)]
    for r in range(world):
        np.testing.assert_allclose(res[r][4], ho, rtol=1e-12)
        if res[r][5] is not None:
            gid, gv = res[r][5]
            assert len(gid) > 0 and np.array_equal(bits(gv), bits(x[gid]))


@pytest.mark.parametrize("world,kind,n", [(3, "elastic3d", 6), (4, "poisson3d", 16)])
def test_multipart_rcm_partition_bit_exact(world, kind, n, built):
    """The graph partitioner through the HIP path: a randomly renumbered grid
    operator, reverse Cuthill-McKee renumbering, nnz-balanced contiguous blocks, N ranks on one
    GPU (host transport, NaN-poisoned ghosts); b, x and residual histories against the oracle's
    setup of the same renumbered matrix with the same offsets."""
    from oracle import oracle as O
    ncycles, max_coarse = 4, 60
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, "rcm:" + kind, n, max_coarse, 0, ncycles, 1, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, 300)
    assert all(res[r][1] == "ok" for r in range(world)), "\n".join(str(res[r][1]) for r in range(world))
    import parallel_amg_amd as pa
    whole, _o, wx = pa.generate_problem(pa.SequentialBackend(1), kind, n)
    whole, wx = pa.permute_problem(whole, wx, 11)
    whole, wx, _perm = pa.rcm_problem(whole, wx)
    _parts, offs, _xp = pa.split_problem(pa.SequentialBackend(world), whole, wx, "nnz")
    M = whole[0]
    Ao = O.CSR(M.rowptr.copy(), M.col.astype(np.int64), M.val.copy(), M.ncols)
    Ho = O.setup(Ao, offsets=offs, max_coarse=max_coarse, agglomerate=0)
    bo = O.spmv(Ao, wx[0])
    xo, ho = Ho.solve(bo, ncycles, res_hist=True)
    bits = lambda a: np.asarray(a, np.float64).view(np.int64)
    assert np.array_equal(bits(np.concatenate([res[r][2] for r in range(world)])), bits(bo))
    assert np.array_equal(bits(np.concatenate([res[r][3] for r in range(world)])), bits(xo))
    for r in range(world):
        np.testing.assert_allclose(res[r][4], ho, rtol=1e-12)


def test_multipart_with_an_empty_part(tmp_path, built):
    """Part 1's rows are all isolated (diagonal only): it forms no aggregates, so it owns no
    row of level 1 — exchanges, tiles and reductions must cope with an empty part."""
    import scipy.io
    import scipy.sparse as sp
    from oracle import oracle as O
    A = O.generate("poisson2d", 20, 20, 1).to_scipy().tolil()
    for i in range(200, 400):
        A[i, :] = 0
        A[:, i] = 0
        A[i, i] = 3.0 + (i % 7)
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    path = str(tmp_path / "iso.mtx")
    scipy.io.mmwrite(path, A.tocoo(), symmetry="symmetric")
    world, ncycles = 2, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, "mtx:" + path, 0, 10, 0, ncycles, 1, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, 300)
    assert all(res[r][1] == "ok" for r in range(world)), "\n".join(str(res[r][1]) for r in range(world))
    Ao = O.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy(), 400)
    Ho = O.setup(Ao, nparts=2, max_coarse=10, agglomerate=0)
    assert Ho.offsets[1][1] == Ho.offsets[1][2]     # part 1 owns no row of level 1
    bo = O.spmv(Ao, O.xstar(400))
    xo, ho = Ho.solve(bo, ncycles, res_hist=True)
    bits = lambda a: np.asarray(a, np.float64).view(np.int64)
    assert np.array_equal(bits(np.concatenate([res[r][2] for r in range(world)])), bits(bo))
    assert np.array_equal(bits(np.concatenate([res[r][3] for r in range(world)])), bits(xo))
