"""The Tiedtke kernels over their geometry: every level count from the smallest accepted one (4) to 66, and 129, on 8 x 5 owned
columns; tile widths of 1 .. 65 columns (a wave edge at 64) at 20 levels; a sub-range with its > ims, which moves the column the
row's leveltop is made from; a tile of more columns than the workspace holds, so that the last chunk of rows is a short one; and a
model top near 400 hPa.  Device against the CPU restatement, 0 differing bits.  (The low-top case is NOT held to the compiled
reference by a fixture of its own; the terrain fixture of tests/test_gpu_tiedtke.py, with a top near 300 hPa, is.)"""
import numpy as np
import pytest

import tiedtke_oracle as T
from icar_amd import convection
from icar_amd.grid import grid_t
from util import parity_record

pytestmark = pytest.mark.gpu
RES = T.TEND + T.OUT2 + ["ktype"]


def compare(c, tile, what, dt=60.0, need_convection=False):
    d = T.device_domain(c)
    A = T.state(c)
    convection.cu_tiedtke(d, dt, *tile)
    T.cu_tiedtke(c, A, dt, tile)
    got = T.device_state(d)
    for k in RES:
        a, b = T.owned(c, got[k], tile), T.owned(c, A[k], tile)
        assert T.bitdiff(a, b) == 0, f"{what}, {k}: {T.bitdiff(a, b)} cells differ"
    d.close()
    n = int((T.owned(c, A["ktype"], tile) == 3).sum())
    assert n > 0 or not need_convection, what
    return n


@pytest.mark.parametrize("first", [4, 20, 36, 52])
def test_every_level_count(first):
    conv = 0
    for nz in list(range(first, min(first + 16, 67))) + ([129] if first == 52 else []):
        c = T.make_case(nx=10, ny=7, nz=nz, seed=100 + nz, depth_max=8000.0)     # 8 x 5 owned columns
        conv += compare(c, T.tile_of(c), f"{nz} levels")
    assert conv > 0 or first < 20, first
    parity_record("tiedtke_columns", f"levels/{first}..{min(first + 15, 66)}", {k: {"bitdiff_cells": 0} for k in RES})


@pytest.mark.parametrize("first", [1, 23, 45])
def test_tile_widths(first):
    c = T.make_case(nx=67, ny=5, nz=20, seed=71, depth_max=8000.0)
    conv = 0
    for w in range(first, min(first + 22, 66)):
        conv += compare(c, (2, 1 + w, 2, 4), f"width {w}")
    assert conv > 0


def test_sub_range_moves_the_leveltop_column():
    p = dict(T.CASES["cu_tiedtke_a_terrain_28x18x40"])
    c = T.make_case(**p)
    its, ite, jts, jte = T.tile_of(c)
    whole, sub = T.state(c), T.state(c)
    T.cu_tiedtke(c, whole, 60.0, (its, ite, jts, jte))
    tile = (ite - 8, ite, jts + 1, jte - 1)
    T.cu_tiedtke(c, sub, 60.0, tile)
    assert T.bitdiff(T.owned(c, whole["tend_th"], tile), T.owned(c, sub["tend_th"], tile)) > 0, "the sub-range's first column gives the same leveltop"
    compare(c, tile, "sub-range", need_convection=True)


def test_short_last_workspace_chunk():
    c = T.make_case(nx=300, ny=222, nz=12, seed=72, depth_max=8000.0)               # 66 600 columns: 218 rows per chunk, then 2
    compare(c, T.tile_of(c), "two chunks", need_convection=True)


def test_low_model_top_against_the_restatement_only():
    c = T.make_case(nx=20, ny=8, nz=30, seed=73, lid=7000.0, base_max=3000.0)
    assert c["pressure_interface"][:, -1].min() > 35000.0, "the model top lies below 350 hPa"
    compare(c, T.tile_of(c), "low top", need_convection=True)
