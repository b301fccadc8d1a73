"""The plan of kernel forms (csrc/forms.hpp), read back on host-only contexts through pop_get_dim("form_<entry>").

Every choice the library makes about kernel forms and schedule is resolved once at create: the library's rule, then the caller's
pop_tuning, then the POP_* environment.  No device is needed to see the outcome.  The expected values below restate the rules as
include/pop_amd.h and DESIGN.md give them (the size rule: more than 2^19 columns on the rank = bandwidth-bound; register kernels
at km = 60 / 62); none is taken from a run of the resolver."""
import os
import re

import pytest

from popcfg import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMIXU_INLINE, VMIXU_SIDE, VMIXU_DEFERRED = 0, 1, 2
BUOY_MARCH, BUOY_PLAIN = 0, 3
INTERIOR_FUSED, INTERIOR_REG = 0, 1


def form_names():
    """the entries of the plan, from the one list that declares them"""
    src = open(os.path.join(ROOT, "pop2-cesm_amd", "csrc", "forms.hpp")).read()
    body = src[src.index("#define POP_FORMS(X)"):src.index("struct Forms {")]
    names = re.findall(r"X\((?:int|bool), (\w+)\)", body)
    assert len(names) > 50 and len(set(names)) == len(names)
    return names


def forms(m):
    return {n: m.dim("form_" + n) for n in form_names()}


def host(pkg, cfg, tuning=None, **kw):
    return pkg.PopModel(cfg, host_only=True, tuning=tuning, **kw)


# ---- both sides of the size rule, at its edge -------------------------------------------------------------------------------------------
def edge_config(nx):
    """one block of nx x 508 cells (+ 2 ghost cells each side), km = 60, del4 + KPP + pcg, no tripole"""
    return named_config("tiny", nx_global=nx, ny_global=508, block_size_x=nx, block_size_y=508, km=60, vmix_choice=3,
                        hmix_tracer=4, hmix_momentum=4, am=-1.0e19, ah=-1.0e18)


@pytest.fixture(scope="module")
def edge(pkg):
    out = []
    for nx in (1020, 1021):
        m = host(pkg, edge_config(nx))
        assert m.dim("nblocks") == 1
        out.append((m.dim("nx_block") * m.dim("ny_block"), forms(m)))
        m.close()
    return out


def test_size_rule_flips_its_entries_and_no_other(edge):
    (n2_small, small), (n2_large, large) = edge
    assert n2_small == 1 << 19 and n2_large > 1 << 19        # 1024 x 512 is the last small grid
    # the look-ahead on a small grid: only beside the resident solve (pcg, diagonal, one rank, <= 8 blocks, <= 250 x 8 chunks of 256 cells)
    resident = n2_small <= 250 * 8 * 256
    governed = {                       # entry: (small, large)
        "xcd_remap": (1, 0),           # XCD bands / linear
        "del4_tile_rows": (0, 4),      # 256 consecutive cells / 64 x 4 patches
        "d2t_fuse": (0, 1), "d2u_fuse": (0, 1),
        "vmixu": (VMIXU_SIDE, VMIXU_DEFERRED),
        "thomas_pair": (0, 1),
        "impvmixu_waves": (2, 1),
        "kpp_col": (1, 31),
        "kpp_ahead": (int(resident), 1),
        # what the mask's bits 3 and 4 select (kpp_col 31): buoydiff + interior as one column march with the sparse boundary-layer kernel,
        # where kpp_col 1 runs the plain 3-D buoydiff and the register interior kernel of km = 60
        "kpp_march": (0, 1), "kpp_sparse": (0, 1), "kpp_buoy": (BUOY_PLAIN, BUOY_MARCH), "kpp_interior": (INTERIOR_REG, INTERIOR_FUSED),
    }
    for name, (s, l) in governed.items():
        assert (small[name], large[name]) == (s, l), name
    assert sorted(n for n in small if small[n] != large[n]) == sorted(governed)
    # and what both sides share at km = 60 with the defaults
    for f in (small, large):
        assert (f["reg_thomas_u"], f["reg_thomas_t"], f["side_stream"], f["del4_side"], f["mom_side"], f["path"], f["fused_ok"]) == (1, 1, 1, 1, 1, 2, 1)
        assert (f["tracer_lds_rows"], f["momentum_lds_rows"], f["red_band"], f["lds_order"], f["land_skip"], f["land_full_steps"]) == (4, 4, 1, 1, 1, 4)


# ---- the level-count rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("km,kw,tuning,reg", [
    (24, {}, None, 0), (60, {}, None, 1), (62, {}, None, 1),
    (60, {"partial_bottom_cells": 1}, None, 1),
    (60, {"partial_bottom_cells": 1}, {"pbc_generic_thomas": 1}, 0),
])
def test_register_kernels_at_km_60_and_62(pkg, km, kw, tuning, reg):
    m = host(pkg, named_config("tiny", km=km, vmix_choice=3, **kw), tuning)
    assert (m.dim("form_reg_thomas_u"), m.dim("form_reg_thomas_t")) == (reg, reg)
    assert (m.dim("thomas_register_velocity"), m.dim("thomas_register_tracers")) == (reg, reg)    # the older names answer from the plan too
    m.close()


# ---- precedence: rule < caller's struct < environment -----------------------------------------------------------------------------------
FOUR_BLOCKS = dict(block_size_x=24, block_size_y=20)
@pytest.mark.parametrize("kw,field,entry,rule,struct,env", [
    ({}, "tracer_lds", "tracer_lds_rows", 4, (8, 8), ("0", 0)),                              # a value
    ({"vmix_choice": 3, "km": 24}, "kpp_ahead", "kpp_ahead", 0, (1, 1), ("0", 0)),          # a rule override (16 blocks: no resident solve, small grid)
    (FOUR_BLOCKS, "solver_unfused", "fused_ok", 1, (1, 0), ("0", 1)),                        # an off switch
])
def test_rule_then_struct_then_environment(pkg, monkeypatch, kw, field, entry, rule, struct, env):
    cfg = named_config("tiny", **kw)
    monkeypatch.delenv("POP_" + field.upper(), raising=False)
    m = host(pkg, cfg)
    assert m.tuning()[field] is None and m.dim("form_" + entry) == rule
    m.close()
    m = host(pkg, cfg, {field: struct[0]})
    assert m.tuning()[field] == struct[0] and m.dim("form_" + entry) == struct[1]
    m.close()
    monkeypatch.setenv("POP_" + field.upper(), env[0])
    m = host(pkg, cfg, {field: struct[0]})
    assert m.tuning()[field] == int(env[0]) and m.dim("form_" + entry) == env[1]
    m.close()


# ---- entries that depend on other entries -----------------------------------------------------------------------------------------------
def test_dependent_entries(pkg):
    del4 = named_config("tiny", hmix_tracer=4, ah=-1.0e21)
    for tuning, want in (({"d2t_fuse": 1}, 1), ({"d2t_fuse": 1, "del4_side": 0}, 0)):
        m = host(pkg, del4, tuning)
        assert (m.dim("form_d2t_fuse"), m.dim("d2t_fused")) == (want, want), tuning
        m.close()
    km60 = named_config("tiny", vmix_choice=3, km=60, hmix_tracer=4, hmix_momentum=4, am=-1.0e21, ah=-1.0e21)
    for side, want in ((None, (1, 1, VMIXU_SIDE, 1)), (0, (0, 0, VMIXU_INLINE, 0))):
        tuning = {"kpp_ahead": 1}
        if side is not None:
            tuning["side_stream"] = side
        m = host(pkg, km60, tuning)
        assert tuple(m.dim("form_" + n) for n in ("side_stream", "kpp_ahead", "vmixu", "mom_side")) == want, tuning
        m.close()


# ---- the solver entries do not depend on the rank ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,tuning,want", [
    ({}, None, {"path": 4, "replicated": 1, "pcsi_two_step_dist": 0}),                                       # pcg, 4 small blocks: replicated
    ({}, {"solver_distributed": 1}, {"path": 3, "replicated": 0, "pcsi_two_step_dist": 0}),
    ({"solver_choice": 3}, {"pcsi_two_step": 1}, {"path": 3, "replicated": 0, "pcsi_two_step_dist": 1}),
])
def test_solver_entries_are_rank_independent(pkg, kw, tuning, want):
    cfg = named_config("wide", block_size_x=528, **kw)
    got = []
    for rank in (0, 1):
        m = host(pkg, cfg, tuning, rank=rank, nranks=2)
        assert m.dim("nblocks") == 2
        got.append({n: m.dim("form_" + n) for n in want})
        m.close()
    assert got[0] == got[1] == want


def test_plan_only_contexts_and_unknown_names_answer_minus_one(pkg):
    m = pkg.PopModel(named_config("tiny"), plan_only=True)
    assert m.dim("form_xcd_remap") == -1
    m.close()
    m = host(pkg, named_config("tiny"))
    assert m.dim("form_no_such_entry") == -1 and m.dim("form_xcd_remap") == 1
    m.close()
