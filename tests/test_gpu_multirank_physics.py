"""Every physics slot of the time step on tiled runs with live halos: `world` processes share cuda:0, each owns one tile of the grid_t
decomposition of the 40 x 28 x 12 case of tests/tiled_step_case.py, and runs icar_hip_step twice (three sub-steps each, diagnostics on,
forced u / v / w / pressure / qv / theta, lsm's update gate open, shut, open) with rad + lsm + pbl + convect + microphysics + advection on
and the halo exchange through the library's host-staged transport, as tests/test_gpu_multirank.py does for advection + microphysics alone.

Checked in every rank:
  * the sub-step count and the model clock after each step() call equal the tiled CPU chain's (tiled_step_case.run: the restatements of
    every slot on this image's host tile, HostTile / HaloComm over gloo where the device exchanges, dt from the oracle's max_courant
    min-reduced over the images -- never read back from the device);
  * the device tile equals that chain bit for bit: every cell of the memory, halo planes included, of every exchanged 3-D field; every
    owned cell of u, v, w, pressure, the scalars that are not exchanged, the surface and radiation outputs, the accumulated precipitation
    and every array of the slots that are on;
  * configurations without a row-coupled scheme and with upwind advection (CONFIGS[..]["star"]): every owned cell also equals the
    one-image device run, byte for byte (rank 0 makes that run and broadcasts it).
That the case reaches what it is there for (convecting columns, land and water in every tile, the gate sequence, tiled /= one image for
the row-coupled schemes, tiled == one image for the others) is asserted without a GPU in tests/test_multirank_physics_inputs.py."""
import copy
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch.distributed as dist

import test_gpu_multirank as MR

pytestmark = pytest.mark.gpu
ROOT = MR.ROOT


@pytest.fixture(scope="module")
def oracle_tables(th_oracle):
    """the oracle's Thompson tables in a file the spawned ranks load (they inherit the environment), removed after the module"""
    where = tempfile.mkdtemp(prefix="icar_thompson_")
    path = os.path.join(where, "tables.npz")
    th_oracle.thompson_tables_save(path)
    os.environ["ICAR_TEST_THOMPSON_TABLES"] = path
    yield path
    os.environ.pop("ICAR_TEST_THOMPSON_TABLES", None)
    shutil.rmtree(where, ignore_errors=True)


def _worker(rank, world, port, name, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dev, hgroup = MR._rendezvous(rank, world)
    try:
        import noah_oracle as N
        import tiled_step_case as TS
        from icar_amd.halo import HaloComm
        from icar_amd.options import options_t
        from icar_amd.time_step import step
        from oracle import orc
        from util import parity_record
        cfg = TS.CONFIGS[name]
        orc.set_num_threads(max(1, min(orc.num_threads(), 16 // world)))  # the ranks share the host
        if cfg["mp"] == "thompson":                                      # the tables the test's own process integrated: 10 s a rank otherwise
            orc.thompson_init_from(*options_t().mp_options.as_arrays(), os.environ["ICAR_TEST_THOMPSON_TABLES"])
        orc.set_math_mode(0)
        tab = N.load_tables() if cfg["lsm"] == "noah" else None
        c, dq, nc = TS.whole_case(orc, cfg, tab)                         # the same whole domain on every rank
        ui, ends = TS.schedule(orc, c)
        opt = TS.options(cfg, c, ui)

        def device_run(g, comm):
            d = TS.device_tile(cfg, opt, TS.cut(c, g), TS.cut(dq, g), g, comm, dev, None if nc is None else TS.cut(nc, g), tab)
            counts, clocks = [], []
            for end in ends:
                counts.append(step(d, end, opt, forced=TS.FORCED, diagnostics=True))
                clocks.append(d.model_time_seconds)
            out = TS.device_fields(cfg, d)
            d.close()
            return counts, clocks, out

        g = TS.grid_of(world, rank + 1, cfg["halo"], c["nz"])
        n_dev, t_dev, got = device_run(g, HaloComm(g, rank + 1))
        # ---- the tiled CPU chain on this image's host tile, exchanging where the device does
        ch = TS.TileChain(orc, cfg, TS.cut(c, g), TS.cut(dq, g), g, ui, None if nc is None else copy.deepcopy(TS.cut(nc, g)), tab)
        n_cpu, t_cpu = TS.run([ch], ends, TS.GlooExchange(ch, rank + 1, hgroup))
        assert n_dev == n_cpu and sum(n_cpu) >= 4, f"sub-steps per step() call: device {n_dev}, CPU chain {n_cpu}"
        assert t_dev == t_cpu, f"model time after each step() call: device {t_dev}, CPU chain {t_cpu}"
        gates = ch.gates
        assert gates[0] and False in gates and True in gates[gates.index(False):], f"lsm's gate: open, shut, open again: {gates}"
        want = TS.chain_fields(cfg, ch)
        lo, gl = TS.owned(g)
        nfields, bad = 0, []
        for group in got:
            assert set(got[group]) == set(want[group]), group
            for k, a in got[group].items():
                b = want[group][k]
                if group != "exchanged":                                 # owned cells; the exchanged fields in every cell of the memory
                    a, b = TS.own(a, lo), TS.own(b, lo)
                n = TS.nbits(a, b)
                print(f"rank {rank} {name} {group}/{k}: {n} of {a.size} values differ from the tiled CPU chain", flush=True)
                nfields += 1
                if n: bad.append(f"{group}/{k}: {n} of {a.size}")
        assert not bad, f"rank {rank}: the device tile differs from the tiled CPU chain in {bad}"
        # ---- the one-image device run (rank 0), where the tiling may not show
        if cfg["star"]:
            ref = None
            if rank == 0:
                n1, t1, one = device_run(TS.grid_of(1, 1, cfg["halo"], c["nz"]), None)
                ref = (n1, t1, one)
            obj = [ref]; dist.broadcast_object_list(obj, src=0); n1, t1, one = obj[0]
            assert n1 == n_dev and t1 == t_dev, f"one image: {n1} sub-steps to {t1}, tiled: {n_dev} to {t_dev}"
            for group in got:
                for k, a in got[group].items():
                    x, y = np.ascontiguousarray(TS.own(a, lo)), np.ascontiguousarray(TS.own(one[group][k], gl))
                    nfields += 1
                    if x.tobytes() != y.tobytes(): bad.append(f"{group}/{k}: {TS.nbits(x, y)} of {x.size}")
            assert not bad, f"rank {rank}: the owned cells of the tiled device run differ from the one-image device run in {bad}"
        parity_record("multirank_physics", f"{name}/world{world}/rank{rank}/{sum(n_cpu)}_substeps", {"all": {"fields": nfields, "bitdiff_cells": 0}})
        print(f"rank {rank} {name}: {nfields} fields compared, 0 bits differ", flush=True)
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,name", [(4, "ysu+bmj"), (4, "noah+ysu"), (4, "simple+tiedtke"), (4, "ysu+nsas+mpdata"), (4, "ysu+nsas@h2"),
                                        (2, "simple+tiedtke"), (8, "ysu+bmj")])
def test_tiled_step_with_every_physics_slot_equals_the_tiled_cpu_chain(oracle_tables, world, name):
    MR._run(_worker, world, name)
