"""Independent pins for the parts of the hot path the reference holds no fixtures for: checks that are
NOT a third restatement of the reference's loops but what the routines are supposed to compute, formed with numpy / scipy:

  * the implicit vertical-mixing solves (vertical_mix.F90:1240-1368 impvmixt, :1563-1658 impvmixt_correct,
    :1750-1868 impvmixu + baroclinic.F90:1077-1129): the tridiagonal system is assembled from VDC / VVC, afac, hfac, H1,
    KMT / KMU and solved by LAPACK's banded solver (scipy.linalg.solve_banded, partial pivoting); the model's solution must
    satisfy the system (residual) and equal LAPACK's;
  * the hydrostatic pressure gradient (pressure_grad.F90:258-301): exactly zero for a horizontally uniform density, and the
    closed form g * a * bouss-weighted trapezoid sum / DXU for a density linear in the i index;
  * horizontal tracer diffusion (hmix_del2.F90:1040-1100, hmix_del4.F90:988-1059): for a field quadratic in the i index the
    Laplacian on the uniform interior of the lat-lon grid is 2a * (east coefficient), a function of j only, so the
    biharmonic operator reduces to a three-point formula in j;
  * the 2-D elliptic system of the barotropic mode (barotropic.F90:417-548, POP_SolversMod.F90; reference statement in
    tests/btrop_ref.py): the solvers' solution against a sparse direct solve of div(HU grad) + centre term assembled from HU, DXU,
    DYU, KMT, KMU alone (check_btrop_solve_against_direct); adjointness of div and grad, sum div = 0, zcurl grad = 0 through the
    operator entry points (check_btrop_operator_properties); the EVP preconditioner as the exact inverse of the five-point operator
    on every solved sub-block, r / centre on the others, and symmetric (check_evp_is_the_local_inverse); the P-CSI eigenvalue
    interval against a dense eigensolve (check_pcsi_interval_contains_the_spectrum, host only); the area-mean surface pressure over
    12 steps (check_mean_sea_level_is_conserved).  Not pinned: the tripole fold (see tests/btrop_ref.py);
  * the momentum right-hand side term by term (advection.F90:1250-1491 advu, baroclinic.F90:1758-1790, hmix_del2.F90:892-927,
    hmix_del4.F90:730-857, vertical_mix.F90:935-1010): advection + Coriolis against the ADVECTIVE form built from the 12-point
    face transports and the column integral of their divergence (check_advu_advective_form: flat, stepped, partial bottom cells with
    DZU weights, implicit Coriolis with different old and current fields), closed forms for uniform and linearly sheared flows
    (check_advu_closed_forms), wind stress and bottom drag (check_wind_stress_and_bottom_drag), del2 / del4 friction of a i^2 and its
    mirror image (check_hdiffu) and of a solid-body rotation, whose truncation figure the metric term DUM sets (check_hdiffu_solid_body);
  * tracer advection, every scheme (advection.F90:2068-2127, :2243-2301, :2313-2676, :2684-3280): a constant stays constant above the
    bottom cell for any flow and everywhere for a flow with no transport through any floor, and such a flow conserves the domain
    sum of a random tracer (check_advt_constant_and_conservation: multi-block, padded, partial bottom cells, passive tracers); the
    upwind3 face values in i, j and k for either flow direction against Lagrange interpolation from positions
    (check_upwind3_face_values).  Not pinned: what lw_lim's limiter does to a field beyond constancy, conservation and
    check_lw_lim_monotone; the tripole fold; hdiffu and the closed forms of advu with partial bottom cells other than through whole
    cells (the min(DZU) / DZU weights of hmix_del2.F90:852-886 act at the bottom level of a stepped neighbourhood only);
  * KPP below the boundary layer and the equation of state under it (vmix_kpp.F90:3575-3621 buoydiff, :1505-1603 and :1774-1986 ri_iwmix,
    :3404-3497 ddmix, :1218-1262 the convective term, :3797-3870 smooth_hblt; state_mod.F90:418-560), against the 40-digit MWJF of
    tests/eos_ref.py (mpmath; derivatives by mpmath.diff of that density) and the closed forms of LMD94: rho, d rho / d T and d rho / d S
    at clipped and unclipped arguments and along the density maximum (check_state_against_mpmath); the displaced-density buoyancy
    difference, the gradient Richardson number, the carry below the bottom, the 1-2-1 smoothing with its end rules, LMD94 (28) and the
    convective term with its strict N2 > 0 test, in VDC of both classes and through tgrid_to_ugrid in VVC, flat, stepped and above a
    partial bottom cell (check_kpp_interior_richardson); both double-diffusion branches on either side of their switches
    (check_kpp_double_diffusion); the 5-point filter of the boundary-layer depth next to land, its bottom clamp and KBL
    (check_kpp_hblt_smoothing).  Not pinned: short-wave absorption and lcheckekmo; the blending of interface KBL - 1 (LMD94 appendix D);
    the floor of HBLT at zt(1) (no closed-form column reaches it); the tidal and latitude-varying backgrounds (NumPy restatements in
    tests/test_gpu_tidal.py, tests/test_gpu_bckgrnd.py); the tripole fold.

The same functions run against the CPU oracle (tests/test_pins_oracle.py, tests/test_btrop_pins_oracle.py, tests/test_dyn_pins_oracle.py,
tests/test_kpp_interior_pins_oracle.py, no GPU) and against the device library through the C ABI (tests/test_gpu_pins.py,
tests/test_gpu_btrop_pins.py, tests/test_gpu_dyn_pins.py, tests/test_gpu_kpp_interior_pins.py): `A` is an adapter with get / set /
run_phase (see OracleAdapter, GpuAdapter)."""
import math

import numpy as np
from scipy.linalg import solve_banded

from common import interior

GRAV = 980.6           # pop_constants.F90:235 (non-CCSMCOUPLED)
THREE_D = ("TRACER", "UVEL", "VVEL", "RHO", "VVC", "KPP_SRC", "UISOP", "VISOP", "WISOP", "GM_SF_SLX", "GM_SF_SLY")


class OracleAdapter:
    def __init__(self, cfg, grid=None):
        from orclib import Oracle
        self.o = Oracle(cfg, grid=grid)
        self.cfg = cfg
        self.km, self.nblocks = self.o.km, self.o.nblocks

    def _arr(self, name, tl, n):
        if name == "VDC":
            return self.o.vdc(n)
        name = {"D4AHF": "D4_AHF", "D4AMF": "D4_AMF"}.get(name, name)
        return (self.o.f3 if name in THREE_D else self.o.f2)(name, tl, n)

    def get(self, name, tl=1, n=0):
        return self._arr(name, tl, n).copy()

    def set(self, name, arr, tl=1, n=0):
        self._arr(name, tl, n)[...] = arr

    def geti(self, name):
        return self.o.i2(name).copy()

    def vert(self, name):
        return self.o.v1(name).copy()       # 1-based with slot 0

    def scalar(self, name):
        return self.o.scalar(name)

    def step(self):
        self.o.step()

    def time_manager(self):
        self.o.L.orc_time_manager(self.o.h)

    def dhdt(self):
        self.o.L.orc_dhdt(self.o.h)

    def run_phase(self, phase):
        if phase in ("vmix", "hmix_tracer", "hmix_momentum", "passive_rhs"):
            return                            # the oracle forms them inside tracer_rhs (every tracer) / momentum_rhs
        self.o.run_phase(phase)

    def correct(self):
        self.o.L.orc_baroclinic_correct_adjust(self.o.h)

    def leapfrog(self):
        return self.o.dim("leapfrogts")

    def state(self, kk, T, S):
        """(rho, d rho / d T, d rho / d S) of the points (T, S) at the pressure of level kk"""
        from orclib import AsModel
        return AsModel(self.o).state(kk, T, S, derivs=True)

    # ---- the 2-D elliptic system: host arrays (nblocks, ny_block, nx_block) in, host arrays out
    def blocks(self):
        """get_block of every block: ib, ie, jb, je (1-based, inclusive), i_glob, j_glob"""
        from orclib import AsModel
        am = AsModel(self.o)
        return [am.get_block(b) for b in am.local_block_ids()]

    def halo(self, a):
        return self.o.halo(a)

    def solver_run(self, x0, b):
        """-> (return code, solution, iterations)"""
        rc, x = self.o.solver_run(x0, b)
        return rc, x, self.o.L.orc_solver_iterations(self.o.h)

    def preconditioner(self, r):
        return self.o.preconditioner(r)

    def operator(self, op, k, a, b=None):
        return self.o.operator(op, k, a, b)

    def btrop_operator(self, x):
        """the nine-point operator on its own (the device library applies it inside its solver kernels only)"""
        return self.o.btrop_operator(x)

    def evp_info(self):
        """the partition and the land flags the implementation holds: (x ranges, y ranges, {(block, jpiece, ipiece): land})"""
        o = self.o
        xnb, ynb = o.evp_info(0), o.evp_info(1)
        xi = [o.evp_info(2, i) for i in range(1, xnb + 2)]
        yi = [o.evp_info(3, j) for j in range(1, ynb + 2)]
        land = {(b, j, i): bool(o.evp_info(4, (b * ynb + j) * xnb + i)) for b in range(o.nblocks) for j in range(ynb) for i in range(xnb)}
        return list(zip(xi[:-1], xi[1:])), list(zip(yi[:-1], yi[1:])), land

    def solver_form(self):
        return None

    def close(self):
        self.o.close()


class GpuAdapter:
    """the device library through the C ABI; vertical grid arrays come from a host-only oracle of the same configuration
    (they are init-time data, compared bit for bit in tests/test_host_grid_parity.py)"""

    def __init__(self, pkg, cfg, grid=None, tuning=None):
        from orclib import Oracle
        self.m = pkg.PopModel(cfg, grid=grid, tuning=tuning)
        self.pkg, self.cfg = pkg, cfg
        self.km, self.nblocks = self.m.km, self.m.nblocks
        o = Oracle(cfg, grid=grid)
        self._vert = {k: o.v1(k).copy() for k in ("dz", "dzw", "dzwr", "bouss", "afac_t", "afac_u", "zt", "zw")}
        o.close()

    def get(self, name, tl=1, n=0):
        return self.m.get({"d4DTE": "d4DTE"}.get(name, name), tl, n)

    def set(self, name, arr, tl=1, n=0):
        self.m.set(name, arr, tl, n)

    def geti(self, name):
        return self.m.geti(name)

    def vert(self, name):
        return self._vert[name]

    def scalar(self, name):
        return self.m.scalar(name)

    def step(self):
        self.m.step()

    def time_manager(self):
        self.m.time_manager()

    def dhdt(self):
        self.m.dhdt()

    def run_phase(self, phase):
        self.m.run_phase(phase)

    def correct(self):
        self.m.baroclinic_correct_adjust()
        self.m.sync()

    def leapfrog(self):
        return self.m.dim("leapfrogts")

    def state(self, kk, T, S):
        return self.m.state(kk, T, S, derivs=True)

    # ---- the 2-D elliptic system: host arrays in, host arrays out, the work done by the device entry points on named fields
    def blocks(self):
        return [self.m.get_block(b) for b in self.m.local_block_ids()]

    def halo(self, a):
        a = np.array(a, dtype=np.float64, order="C")
        self.m.halo_update_host(a)
        return a

    def solver_run(self, x0, b):
        """POP_SolversRun on RHS and PSURF(newtime) in whatever form the model dispatches to (see solver_form)"""
        self.m.set("RHS", b)
        self.m.set("PSURF", x0, 2)
        try:
            self.m.solver_run()
            rc = 0
        except self.pkg.PopError:
            rc = 1
        return rc, self.m.get("PSURF", 2), self.m.solver_diagnostics()[0]

    def preconditioner(self, r):
        self.m.set("RHS", r)
        self.m.solver_preconditioner("RHS", "DH")
        return self.m.get("DH")

    def operator(self, op, k, a, b=None):
        if op == "grad":
            self.m.set("PSURF", a)
            self.m.operator("grad", k, "PSURF", o1="GRADPX", o2="GRADPY")
            return self.m.get("GRADPX"), self.m.get("GRADPY")
        self.m.set("UBTROP", a)
        self.m.set("VBTROP", b)
        self.m.operator(op, k, "UBTROP", "VBTROP", o1="DH")
        return self.m.get("DH")

    def solver_form(self):
        """(solver_path, pcg_persist_used) of the last solve: 1 operation by operation / 2 fused; the resident launch or not"""
        return self.m.dim("solver_path"), self.m.dim("pcg_persist_used")

    def close(self):
        self.m.close()


def _prepare(A, nsteps=2):
    """a developed state, then the step parameters of a leapfrog step"""
    for _ in range(nsteps):
        A.step()
    A.time_manager()
    assert A.leapfrog() == 1
    return 2.0 * A.scalar("dtt")          # c2dtt = c2dtu (step_mod.F90:302-320; dt(k) = dtt, dtu = dtt)


def _tridiag_solve(h, a_face, kbot, rhs_h):
    """LAPACK solution of the columns' systems.  Row k (1-based, k <= kbot):
         -A(k-1) x(k-1) + (h(k) + A(k-1) + A(k)) x(k) - A(k) x(k+1) = rhs_h(k),   A(0) = A(kbot) = 0
    (what the recurrences of vertical_mix.F90:1263-1368 eliminate); rows below the bottom: x = 0.
    h, a_face, rhs_h: (km, ncol); kbot: (ncol,).  Returns x (km, ncol) and the residual of a given solution."""
    km, ncol = h.shape
    x = np.zeros((km, ncol))
    for c in range(ncol):
        kb = int(kbot[c])
        if kb < 1:
            continue
        A = a_face[:kb, c].copy()
        A[kb - 1] = 0.0
        Am = np.concatenate(([0.0], A[:-1]))
        ab = np.zeros((3, kb))
        ab[0, 1:] = -A[:-1]
        ab[1, :] = h[:kb, c] + Am + A
        ab[2, :-1] = -A[:-1]
        x[:kb, c] = solve_banded((1, 1), ab, rhs_h[:kb, c])
    return x


def _tridiag_residual(h, a_face, kbot, rhs_h, x):
    km, ncol = h.shape
    k = np.arange(1, km + 1)[:, None]
    A = np.where(k < kbot[None, :], a_face, 0.0)            # no flux through the bottom face or below
    Am = np.vstack([np.zeros((1, ncol)), A[:-1]])
    xp = np.vstack([x[1:], np.zeros((1, ncol))])
    xm = np.vstack([np.zeros((1, ncol)), x[:-1]])
    r = -Am * xm + (h + Am + A) * x - A * xp - rhs_h
    r = np.where(k <= kbot[None, :], r, x)                  # below the bottom the solution itself must vanish
    return np.where(kbot[None, :] > 0, r, 0.0)              # land columns: the reference leaves don't-care values at k = 1


def _thickness(A, kind):
    """level thicknesses per interior column, (km, ncol): dz(k), or with partial bottom cells (grid.F90:926-951) DZT = DZBC at
    the bottom level of a T column, and DZU = the minimum of the four surrounding DZT at a U column -- formed here from KMT and
    DZBC alone, independently of what either implementation stores"""
    return _cols(_thickness4(A, kind))


def _thickness4(A, kind):
    """_thickness as (nblocks, km, ny, nx), ghost cells included (DZU: all but the last ghost row and column)"""
    km = A.km
    dz = A.vert("dz")[1:km + 1]
    kmt = A.geti("KMT")
    if not A.cfg.partial_bottom_cells:
        return np.broadcast_to(dz[None, :, None, None], (kmt.shape[0], km) + kmt.shape[1:]).copy()
    dzbc = A.get("DZBC")
    k = np.arange(1, km + 1)[None, :, None, None]
    dzt = np.where(k == kmt[:, None], dzbc[:, None], dz[None, :, None, None])          # (nblocks, km, ny, nx), ghosts included
    if kind == "T":
        return dzt
    dzu = dzt.copy()
    dzu[..., :-1, :-1] = np.minimum(np.minimum(dzt[..., :-1, :-1], dzt[..., :-1, 1:]), np.minimum(dzt[..., 1:, :-1], dzt[..., 1:, 1:]))
    return dzu


def _faces(dzc, coef):
    """A(k) = coefficient(k) / (distance between the centres of levels k and k + 1) for per-column thicknesses dzc (km, ncol)"""
    below = np.vstack([dzc[1:], np.zeros((1, dzc.shape[1]))])
    return coef / (0.5 * (dzc + below))


def _cols(a3):
    """(nblocks, km, ny, nx) interior -> (km, ncol)"""
    b = interior(a3)
    return np.moveaxis(b, 1, 0).reshape(b.shape[1], -1)


def check_impvmixt(A, rng, tol_res=1e-13, tol_sol=1e-12):
    """impvmixt (predictor, PSFC = PSURF(cur)): T(new) = T(old) + x, x from the tridiagonal system with right-hand side
    hfac_t(k) * rhs(k) and H1 = hfac_t(1) + PSFC / (grav c2dtt(1)) on the diagonal of the first row"""
    c2dt = _prepare(A)
    km = A.km
    dz, afac = A.vert("dz")[1:km + 1], A.vert("afac_t")[1:km + 1]
    kmt = A.geti("KMT")
    # KPP keeps one diffusivity per tracer class; without double diffusion the two classes hold the same values (the library then
    # keeps ONE array for both), so distinct values per class are pinned with ldbl_diff only
    nset = 2 if A.cfg.vmix_choice == 3 else 1
    nvdc = 2 if (A.cfg.vmix_choice == 3 and A.cfg.ldbl_diff) else 1
    shp = A.get("TRACER", 2, 0).shape
    ps = 40.0 * GRAV * (rng.random(A.get("PSURF", 1).shape) - 0.5)       # +- 20 cm of sea level
    A.set("PSURF", ps, 1)
    vdc = [0.05 + 50.0 * rng.random(A.get("VDC", 0, n).shape) ** 3 for n in range(2)]
    for n in range(nset):
        A.set("VDC", vdc[n if nvdc == 2 else 0], 0, n)
    rhs = [10.0 * (rng.random(shp) - 0.5) for _ in range(2)]
    told = [A.get("TRACER", 0, n) for n in range(2)]
    for n in range(2):
        A.set("TRACER", rhs[n], 2, n)
    A.run_phase("impvmixt")
    worst = 0.0
    for n in range(2):
        out = A.get("TRACER", 2, n)
        v = vdc[n if nvdc == 2 else 0]
        a_face = afac[:, None] * _cols(v[:, 1:km + 1])
        h = np.repeat((dz / c2dt)[:, None], a_face.shape[1], axis=1)
        if A.cfg.partial_bottom_cells:      # the same system on the columns' own thicknesses
            dzc = _thickness(A, "T")
            a_face, h = _faces(dzc, _cols(v[:, 1:km + 1])), dzc / c2dt
        rhs_h = h * _cols(rhs[n])
        h[0] = h[0] + interior(ps).reshape(-1) / (GRAV * c2dt)
        kb = interior(kmt).reshape(-1)
        x = _cols(out) - _cols(told[n])
        scale = np.abs(rhs_h).max()
        res = np.abs(_tridiag_residual(h, a_face, kb, rhs_h, x)).max() / scale
        ref = _tridiag_solve(h, a_face, kb, rhs_h)
        err = np.abs(np.where(kb[None, :] > 0, x - ref, 0.0)).max() / np.abs(ref).max()
        assert res <= tol_res, "impvmixt tracer %d: residual %.3e" % (n, res)
        assert err <= tol_sol, "impvmixt tracer %d: differs from LAPACK by %.3e" % (n, err)
        worst = max(worst, res, err)
    assert (interior(kmt) == 0).any() and (interior(kmt) > 0).any()     # land and ocean columns were both checked
    return worst


def check_impvmixt_correct(A, rng, tol_res=1e-13, tol_sol=1e-12):
    """impvmixt_correct (baroclinic.F90:1261-1330 + vertical_mix.F90:1563-1658), pressure-averaging leapfrog step:
    T(new) += x with the same matrix (PSFC = PSURF(new)) and the right-hand side hfac_t(1) * RHS1 in the first row only,
    RHS1 = ((2 T(cur) - T(old)) (P(cur) - P(old)) - T(new) (P(new) - P(cur))) / (grav dz(1)) at the surface level"""
    c2dt = _prepare(A)
    assert A.cfg.lpressure_avg == 1
    km = A.km
    dz, afac = A.vert("dz")[1:km + 1], A.vert("afac_t")[1:km + 1]
    kmt = A.geti("KMT")
    # KPP keeps one diffusivity per tracer class; without double diffusion the two classes hold the same values (the library then
    # keeps ONE array for both), so distinct values per class are pinned with ldbl_diff only
    nset = 2 if A.cfg.vmix_choice == 3 else 1
    nvdc = 2 if (A.cfg.vmix_choice == 3 and A.cfg.ldbl_diff) else 1
    shp2 = A.get("PSURF", 1).shape
    P = [40.0 * GRAV * (rng.random(shp2) - 0.5) for _ in range(3)]
    for tl in range(3):
        A.set("PSURF", P[tl], tl)
    vdc = [0.05 + 50.0 * rng.random(A.get("VDC", 0, n).shape) ** 3 for n in range(2)]
    for n in range(nset):
        A.set("VDC", vdc[n if nvdc == 2 else 0], 0, n)
    tn = [A.get("TRACER", 1, n) * (1.0 + 0.05 * (rng.random(A.get("TRACER", 1, n).shape) - 0.5)) for n in range(2)]
    tc = [A.get("TRACER", 1, n) for n in range(2)]
    to = [A.get("TRACER", 0, n) for n in range(2)]
    for n in range(2):
        A.set("TRACER", tn[n], 2, n)
    A.correct()
    worst = 0.0
    for n in range(2):
        out = A.get("TRACER", 2, n)
        v = vdc[n if nvdc == 2 else 0]
        a_face = afac[:, None] * _cols(v[:, 1:km + 1])
        h = np.repeat((dz / c2dt)[:, None], a_face.shape[1], axis=1)
        if A.cfg.partial_bottom_cells:
            dzc = _thickness(A, "T")
            a_face, h = _faces(dzc, _cols(v[:, 1:km + 1])), dzc / c2dt
        kb = interior(kmt).reshape(-1)
        rhs1 = ((2.0 * tc[n][:, 0] - to[n][:, 0]) * (P[1] - P[0]) - tn[n][:, 0] * (P[2] - P[1])) / (GRAV * dz[0])
        rhs_h = np.zeros_like(h)
        rhs_h[0] = h[0] * np.where(kb > 0, interior(rhs1).reshape(-1), 0.0)
        h[0] = h[0] + interior(P[2]).reshape(-1) / (GRAV * c2dt)
        x = _cols(out) - _cols(tn[n])
        scale = np.abs(rhs_h).max()
        res = np.abs(_tridiag_residual(h, a_face, kb, rhs_h, x)).max() / scale
        ref = _tridiag_solve(h, a_face, kb, rhs_h)
        # x is a difference of O(20) numbers: its rounding floor is eps * |T| / |x|
        floor = 4.0e-16 * np.abs(_cols(tn[n])).max() / np.abs(ref).max()
        err = np.abs(np.where(kb[None, :] > 0, x - ref, 0.0)).max() / np.abs(ref).max()
        assert res <= tol_res + 10 * floor, "impvmixt_correct tracer %d: residual %.3e" % (n, res)
        assert err <= tol_sol + 10 * floor, "impvmixt_correct tracer %d: differs from LAPACK by %.3e" % (n, err)
        worst = max(worst, res, err)
    return worst


def check_impvmixu(A, rng, tol_sol=1e-12):
    """impvmixu + the tail of baroclinic_driver: x from the tridiagonal system (hfac_u, afac_u VVC, bottom at KMU), then
    U(new) = U(old) + x minus its depth mean (sum over k of U dz / HU) on k <= KMU, 0 below"""
    c2dt = _prepare(A)
    km = A.km
    dz, afac = A.vert("dz")[1:km + 1], A.vert("afac_u")[1:km + 1]
    kmu = A.geti("KMU")
    vvc = 0.5 + 100.0 * rng.random(A.get("VVC").shape) ** 3
    A.set("VVC", vvc)
    shp = vvc.shape
    rhs = [5.0 * (rng.random(shp) - 0.5) for _ in range(2)]
    old = [A.get(f, 0) for f in ("UVEL", "VVEL")]
    hur = A.get("HUR")
    for f, r in zip(("UVEL", "VVEL"), rhs):
        A.set(f, r, 2)
    A.run_phase("impvmixu")
    worst = 0.0
    kb = interior(kmu).reshape(-1)
    klev = np.arange(1, km + 1)[:, None]
    for f, r, o in zip(("UVEL", "VVEL"), rhs, old):
        out = _cols(A.get(f, 2))
        a_face = afac[:, None] * _cols(vvc)
        h = np.repeat((dz / c2dt)[:, None], a_face.shape[1], axis=1)
        dzc = np.repeat(dz[:, None], a_face.shape[1], axis=1)
        if A.cfg.partial_bottom_cells:
            dzc = _thickness(A, "U")
            a_face, h = _faces(dzc, _cols(vvc)), dzc / c2dt
            # the depth the mean divides by is the sum of the column's thicknesses (grid.F90:1011-1014)
            hu = np.where(klev <= kb[None, :], dzc, 0.0).sum(axis=0)
            assert np.allclose(np.where(kb > 0, hu * interior(hur).reshape(-1), 1.0), 1.0, rtol=1e-13)
        x = _tridiag_solve(h, a_face, kb, h * _cols(r))
        unew = _cols(o) + x
        mean = (unew * dzc).sum(axis=0) * interior(hur).reshape(-1)
        expect = np.where(klev <= kb[None, :], unew - mean[None, :], 0.0)
        err = np.abs(out - expect).max() / np.abs(expect).max()
        assert err <= tol_sol, "%s after impvmixu: differs from the LAPACK-based value by %.3e" % (f, err)
        worst = max(worst, err)
    assert (kb == 0).any() and (kb > 0).any()
    return worst


def _quiet(A):
    """no flow, flat sea surface, no wind: only the pressure-gradient / diffusion terms under test remain"""
    z3 = np.zeros(A.get("UVEL", 1).shape)
    for tl in range(3):
        A.set("UVEL", z3, tl)
        A.set("VVEL", z3, tl)
        A.set("PSURF", np.zeros(A.get("PSURF", 1).shape), tl)
    for n in range(2):
        A.set("SMF", np.zeros(A.get("SMF", 1, n).shape), 1, n)


def _forces(A, c2dt):
    """FX, FY of clinic from U, V(new) = (FX + w FY, FY - w FX) c2dtu / (1 + w^2), w = c2dtu beta FCOR (baroclinic.F90:1013-1045)"""
    u, v = A.get("UVEL", 2), A.get("VVEL", 2)
    if not A.cfg.impcor:
        return u / c2dt, v / c2dt
    w = (c2dt * (1.0 / 3.0) * A.get("FCOR"))[:, None]
    return (u - w * v) / c2dt, (v + w * u) / c2dt


def check_gradp(A, tol=1e-12):
    c2dt = _prepare(A)
    km = A.km
    _quiet(A)
    kmu = A.geti("KMU")
    shp = A.get("RHO", 1).shape
    prof = 1.0 + np.round(40.0 * np.arange(km) / km) * 2.0 ** -10    # rho(z), g/cm^3, exactly representable
    # (1) horizontally uniform density: no pressure force anywhere, exactly
    for tl in range(3):
        A.set("RHO", np.broadcast_to(prof[None, :, None, None], shp).copy(), tl)
    A.run_phase("hmix_momentum")
    A.run_phase("momentum_rhs")
    for f in ("UVEL", "VVEL"):
        assert np.abs(interior(A.get(f, 2))).max() == 0.0, "gradp of rho(z) is not exactly zero (%s)" % f
    assert np.abs(interior(A.get("ZX"))).max() == 0.0 and np.abs(interior(A.get("ZY"))).max() == 0.0
    # (2) rho = rho(z) + a * (i index within the block): grad_x = a bouss(k) / DXU exactly, grad_y = 0;
    # hydrostatic sum (pressure_grad.F90:280-296): SUMX(k) = SUMX(k-1) + dzw(k-1) grav 0.5 (gx(k) + gx(k-1)), gx(0) = gx(1)
    a = 2.0 ** -7                                                   # large on purpose: the check is arithmetic, and a difference of
                                                                    # densities must stay far above their rounding (4e-16)
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :]
    for tl in range(3):
        A.set("RHO", prof[None, :, None, None] + a * ii + np.zeros(shp), tl)
    A.run_phase("hmix_momentum")
    A.run_phase("momentum_rhs")
    fx, fy = _forces(A, c2dt)
    bouss, dzw = A.vert("bouss")[1:km + 1], A.vert("dzw")[0:km]
    gx = a * bouss[None, :, None, None] / A.get("DXU")[:, None]
    gxm = np.concatenate([gx[:, :1], gx[:, :-1]], axis=1)
    sumx = np.cumsum(dzw[None, :, None, None] * GRAV * 0.5 * (gx + gxm), axis=1)
    ocean = np.arange(1, km + 1)[None, :, None, None] <= kmu[:, None]
    expect = np.where(ocean, -sumx, 0.0)
    # the i index is linear inside a block only: leave out the two columns next to a block's eastern edge
    sel = (slice(None), slice(None), slice(2, -2), slice(2, -4))
    err = np.abs(fx[sel] - expect[sel]).max() / np.abs(expect[sel]).max()
    assert err <= tol, "gradp of a density linear in x: FX differs from the closed form by %.3e" % err
    assert np.abs(fy[sel]).max() <= tol * np.abs(expect[sel]).max(), "gradp of a density linear in x: FY is not zero"
    assert ocean[sel].any() and (~ocean[sel]).any()
    return err


def check_hdifft(A, tol=None):
    """tracer_update with nothing but horizontal diffusion acting (no flow, level-independent tracers, no fluxes):
    T(new) = c2dtt * HDTK.  T = a i^2 (i = index within the block) away from land and block edges:
      del2:  HDTK = ah * 2a * DTE(j)                                    (DTE = DTW on the lat-lon grid, hmix_del2.F90:619-634)
      del4:  D2 = AHF * 2a * DTE(j);  HDTK = ah * (DTN (D2(j+1) - D2(j)) + DTS (D2(j-1) - D2(j)))   (hmix_del4.F90:1021-1059)"""
    c2dt = _prepare(A)
    km = A.km
    _quiet(A)
    del4 = A.cfg.hmix_tracer == 4
    # rounding floor: the first Laplacian cancels 2i of 2i + 1 parts (i up to ~50), the second differences first
    # Laplacians that agree to ~1e-3 between neighbouring rows: 1e-16 * 1e2 (* 1e3) -- a wrong coefficient shows at O(1)
    tol = tol or (1e-9 if del4 else 1e-12)
    pre = "d4" if del4 else ""
    dte, dtw, dtn, dts = (A.get(pre + n) for n in ("DTE", "DTW", "DTN", "DTS"))
    kmt = A.geti("KMT")
    shp = A.get("TRACER", 1, 0).shape
    a = 2.0 ** -6
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :]
    field = [a * ii * ii + np.zeros(shp), 0.5 * a * ii * ii + 0.01 + np.zeros(shp)]
    for n in range(2):
        for tl in range(3):
            A.set("TRACER", field[n], tl, n)
        A.set("STF", np.zeros(kmt.shape), 1, n)
    if A.cfg.vmix_choice == 3:
        for n in range(2):
            A.set("KPP_SRC", np.zeros(shp), 1, n)
    A.dhdt()
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    # cells whose whole stencil (radius 2 for del4 incl. the land test) is full-depth ocean inside one block
    full = (kmt == km)
    ok = full.copy()
    r = 3
    for dj in range(-r, r + 1):
        for di in range(-r, r + 1):
            ok &= np.roll(np.roll(full, dj, axis=1), di, axis=2)
    ok[:, :r + 2, :] = False; ok[:, -(r + 2):, :] = False; ok[:, :, :r + 2] = False; ok[:, :, -(r + 2):] = False
    assert ok.any(), "no open-ocean patch in this configuration"
    ah = A.cfg.ah
    worst = 0.0
    for n, amp in ((0, a), (1, 0.5 * a)):
        out = A.get("TRACER", 2, n) / c2dt
        if del4:
            ahf = A.get("D4AHF") if A.cfg.lvariable_hmix else np.ones(dte.shape)
            d2 = ahf * 2.0 * amp * dte
            expect = ah * (dtn * (np.roll(d2, -1, axis=1) - d2) + dts * (np.roll(d2, 1, axis=1) - d2))
        else:
            expect = ah * 2.0 * amp * dte
        assert np.abs(dte - dtw)[ok].max() <= 1e-15 * np.abs(dte)[ok].max()
        for k in range(km):
            e = np.abs(out[:, k] - expect)[ok].max() / np.abs(expect)[ok].max()
            worst = max(worst, e)
    assert worst <= tol, "hdifft of a quadratic field differs from the closed form by %.3e" % worst
    return worst


# ------------------------------------------------------------------------------------------------------------------
# KPP (vmix_kpp.F90) against Large, McWilliams & Doney (1994): the published similarity functions, the boundary-layer
# shape function and the bulk-Richardson-number depth on a two-layer column.  Nothing below evaluates the model's own
# formulas: the expected values are written from the paper (appendix B for phi_m, phi_s and their constants) and from the
# geometry of the column.
# ------------------------------------------------------------------------------------------------------------------
VONKAR, EPSSFC, RICR = 0.4, 0.1, 0.3           # von Karman constant, surface-layer extent, critical bulk Ri (LMD94 2, 21)
ZETA_M, ZETA_S, A_M, C_M, A_S, C_S = -0.2, -1.0, 1.26, 8.38, -28.86, 98.96    # LMD94 (B1), (B2)
CSTAR = 10.0                                   # non-local transport, LMD94 (20)
KPP_EPS = 1.0e-10                              # vmix_kpp.F90:104


def phi_m(zeta):
    """LMD94 (B1): 1 + 5 zeta | (1 - 16 zeta)^-1/4 | (a_m - c_m zeta)^-1/3"""
    z = np.asarray(zeta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(z >= 0.0, 1.0 + 5.0 * z, np.where(z >= ZETA_M, (1.0 - 16.0 * z) ** -0.25, (A_M - C_M * z) ** (-1.0 / 3.0)))


def phi_s(zeta):
    """LMD94 (B1): 1 + 5 zeta | (1 - 16 zeta)^-1/2 | (a_s - c_s zeta)^-1/3"""
    z = np.asarray(zeta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(z >= 0.0, 1.0 + 5.0 * z, np.where(z >= ZETA_S, (1.0 - 16.0 * z) ** -0.5, (A_S - C_S * z) ** (-1.0 / 3.0)))


def _patch(kmt, km, r=3):
    """columns whose neighbourhood of radius r is full-depth ocean inside one block"""
    full = (kmt == km)
    ok = full.copy()
    for dj in range(-r, r + 1):
        for di in range(-r, r + 1):
            ok &= np.roll(np.roll(full, dj, axis=1), di, axis=2)
    ok[:, :r + 2, :] = False; ok[:, -(r + 2):, :] = False; ok[:, :, :r + 2] = False; ok[:, :, -(r + 2):] = False
    assert ok.any(), "no open-ocean patch in this configuration"
    return ok


def _two_layer(A, kstar, t1, t2, salt=35.0, u1=0.0, u2=0.0):
    """levels 1 .. kstar-1: temperature t1, velocity (u1, 0); levels kstar .. km: t2, (u2, 0); uniform salinity (model units)"""
    shp = A.get("TRACER", 1, 0).shape
    km = A.km
    lev = np.arange(1, km + 1)[None, :, None, None]
    T = np.where(lev < kstar, t1, t2) + np.zeros(shp)
    U = np.where(lev < kstar, u1, u2) + np.zeros(shp)
    for tl in range(3):
        A.set("TRACER", T, tl, 0)
        A.set("TRACER", np.full(shp, salt), tl, 1)
        A.set("UVEL", U, tl)
        A.set("VVEL", np.zeros(shp), tl)
    return T


def _rho_of_uniform_column(A, temp, salt):
    """in-situ density of (temp, salt) at the pressure of every level: the model's own `state` phase on a uniform column.
    (The equation of state is compared with the oracle level by level in the phase-parity tests; here it only supplies
    the buoyancy jump and the surface expansion coefficient the closed forms need.)"""
    shp = A.get("TRACER", 1, 0).shape
    keep = [(A.get("TRACER", tl, n), tl, n) for tl in range(3) for n in range(2)]
    for tl in range(3):
        A.set("TRACER", np.full(shp, temp), tl, 0)
        A.set("TRACER", np.full(shp, salt), tl, 1)
    A.run_phase("state")
    tl_new = 2
    rho = A.get("RHO", tl_new)
    for arr, tl, n in keep:
        A.set("TRACER", arr, tl, n)
    return rho


def _surface_buoyancy_flux(A, t1, salt, stf_t, ok):
    """Bo = -g (d rho / d T) STF_T / rho at the surface level (LMD94 (A3b), no salt flux): the derivative by central differences
    of the density the model's `state` phase returns"""
    d = 2.0 ** -6
    rp, rm, r0 = (_rho_of_uniform_column(A, t, salt)[:, 0][ok] for t in (t1 + d, t1 - d, t1))
    drdt = (rp - rm) / (2.0 * d)
    return float(np.median(-GRAV * drdt * stf_t / r0)), float(np.abs(drdt - np.median(drdt)).max())


def _kpp_setup(A, kstar, t1, t2, ustar, stf_t, u1=0.0, u2=0.0, salt=35.0):
    _prepare(A)
    for tl in range(3):
        A.set("PSURF", np.zeros(A.get("PSURF", 1).shape), tl)
    _two_layer(A, kstar, t1, t2, salt, u1, u2)
    kmt = A.geti("KMT")
    z2 = np.zeros(kmt.shape)
    for name in ("SMF", "SMFT"):                 # |tau| / rho_0 = ustar^2 (vmix_kpp.F90:2177: USTAR = sqrt(|SMFT|); the stress at U and at T points
        A.set(name, z2 + ustar * ustar, 1, 0)    # are separate forcing fields, forcing_ws.F90:307)
        A.set(name, z2, 1, 1)
    A.set("STF", z2 + stf_t, 1, 0)
    A.set("STF", z2, 1, 1)
    return kmt


def _kpp_run(A):
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")


def check_kpp_scales_and_shape(A, regime, nu0=0.0, tol=1e-7):
    """Inside the boundary layer the diffusivity at the interface of depth d = zw(k) is K_x = h w_x(sigma) G(sigma), sigma = d / h
    (LMD94 (10)), w_x = kappa ustar / phi_x(zeta), zeta = min(sigma, eps) h kappa Bf / ustar^3 (LMD94 (13); the reference clips
    sigma at eps in every regime, vmix_kpp.F90:3085), G(sigma) = sigma (1 + a2 sigma + a3 sigma^2) with G(1) = nu(h) / (h w_x(1)),
    dG(1) = 0 for a depth-independent interior nu (LMD94 (17), (18), (D5)): a2 = -2 + 3 G(1), a3 = 1 - 2 G(1).
    Non-local term of the tracer equation (LMD94 (20)): K_s gamma_s = C* kappa (c_s kappa eps)^1/3 G(sigma) * surface flux in
    unstable forcing, none in stable forcing.  `regime`: 'stable' | 'weak' | 'strong' picks the forcing; the similarity regime
    reached (the branch of phi) is asserted.  Interior: no shear-instability term (lrich = 0), uniform background nu0; the shear-instability
    term, the convective term and double diffusion below the boundary layer are pinned by check_kpp_interior_richardson and
    check_kpp_double_diffusion."""
    km = A.km
    kstar = 9
    ustar, stf = {"stable": (0.5, 1.0e-4), "weak": (2.0, -1.0e-3), "strong": (0.6, -6.0e-3)}[regime]
    t1, t2, salt = 18.0, 8.0, 0.035
    kmt = _kpp_setup(A, kstar, t1, t2, ustar, stf, salt=salt)
    ok = _patch(kmt, km)
    bo, spread = _surface_buoyancy_flux(A, t1, salt, stf, ok)
    assert spread <= 1e-12
    if bo >= 0.0:
        bo = bo + 2.0 * KPP_EPS                             # the reference's regularisation of stable forcing, applied in the level march of
                                                            # bldepth and again after it (vmix_kpp.F90:2418, 2755; no short wave)
    u3 = ustar ** 3 + KPP_EPS                               # and of zeta (:3297)
    _kpp_run(A)
    hblt, kbl = A.get("HBLT"), A.geti("KBL")
    zw, zt, dz = A.vert("zw"), A.vert("zt"), A.vert("dz")
    h = hblt[ok]                                            # every column of the patch with its own depth
    assert np.abs(h - np.median(h)).max() <= 1e-6 * np.median(h) and (kbl[ok] == kbl[ok].flat[0]).all()
    KB = int(kbl[ok].flat[0])
    assert KB >= 5, "boundary layer too shallow for the check (KBL = %d)" % KB
    zeta_sl = EPSSFC * h * VONKAR * bo / u3
    if regime == "stable":
        assert zeta_sl.min() > 0.0
    elif regime == "weak":
        assert ZETA_M < zeta_sl.min() and zeta_sl.max() < 0.0     # both phi on their (1 - 16 zeta) branch
    else:
        assert zeta_sl.max() < ZETA_S                       # both phi on their convective (a - c zeta)^1/3 branch
    worst = 0.0
    cg = CSTAR * VONKAR * (C_S * VONKAR * EPSSFC) ** (1.0 / 3.0)
    vdc = [A.get("VDC", 1, n) for n in range(2)]
    vvc = A.get("VVC")
    src = A.get("KPP_SRC", 1, 0)
    w1 = {"m": VONKAR * ustar / phi_m(zeta_sl), "s": VONKAR * ustar / phi_s(zeta_sl)}
    nu = {"m": nu0 * A.cfg.Prandtl, "s": nu0}
    # the viscosity reaches U points as the area-weighted mean of the four surrounding T cells (grid.F90 tgrid_to_ugrid):
    # a horizontally uniform value is multiplied by the sum of the weights
    ta, ua = A.get("TAREA"), A.get("UAREA")
    t2u = (0.25 * (ta + np.roll(ta, -1, axis=2) + np.roll(ta, -1, axis=1) + np.roll(np.roll(ta, -1, axis=1), -1, axis=2)) / ua)[ok]
    g_prev = 0.0
    for k in range(1, KB - 1):                              # interfaces 1 .. KBL-2: pure boundary-layer values (LMD94 appendix D changes KBL-1)
        sig = zw[k] / h
        zeta = np.minimum(sig, EPSSFC) * h * VONKAR * bo / u3
        G = {}
        for x, phi in (("m", phi_m), ("s", phi_s)):
            wx = VONKAR * ustar / phi(zeta)
            g1 = nu[x] / (h * w1[x])
            G[x] = sig * (1.0 + sig * ((-2.0 + 3.0 * g1) + (1.0 - 2.0 * g1) * sig))
            expect = h * wx * G[x] * (t2u if x == "m" else 1.0)
            got = (vvc[:, k - 1] if x == "m" else vdc[0][:, k])[ok]          # VDC carries the levels 0 .. km+1, VVC 1 .. km
            worst = max(worst, float((np.abs(got - expect) / expect).max()))
        assert np.array_equal(vdc[0][:, k][ok], vdc[1][:, k][ok])
        # non-local source of level k: STF / dz(k) * (K gamma (top) - K gamma (bottom)), K gamma = cg G_s(sigma) when unstable
        gam = cg * G["s"] if bo < 0.0 else 0.0
        expect = stf / dz[k] * (g_prev - gam)
        got = src[:, k - 1][ok]
        if bo < 0.0:
            worst = max(worst, float(np.abs(got - expect).max() / abs(stf / dz[k] * cg)))
        else:
            assert np.abs(got).max() == 0.0
        g_prev = gam
    assert worst <= tol, "KPP boundary-layer coefficients differ from the published forms by %.3e (%s, nu0 = %g)" % (worst, regime, nu0)
    return worst


def check_kpp_hblt_two_layer(A, tol=2e-7):
    """Boundary-layer depth of a two-layer column (LMD94 (21)): the bulk Richardson number is 0 at every level of the upper
    layer and Ri* = (d - eps d / 2) db / |dV|^2 at the first level of the lower layer (d = zt(k*), db the buoyancy jump at that
    level's pressure, dV the velocity jump; no local stratification below the jump, so no unresolved-shear term).  The
    reference interpolates Ri_b(z) by the parabola through the last three levels (vmix_kpp.F90:2600-2640): with Ri_b = 0
    at the two upper ones its root is  h = zt(k*-1) + (zt(k*) - zt(k*-1)) sqrt(Ri_c / Ri*)."""
    km = A.km
    kstar, t1, t2, salt = 8, 16.0, 15.0, 0.035
    du = 14.0
    kmt = _kpp_setup(A, kstar, t1, t2, 1.0, -1.0e-4, u1=du, u2=0.0, salt=salt)
    ok = _patch(kmt, km)
    ra = _rho_of_uniform_column(A, t1, salt)[:, kstar - 1][ok]
    rb = _rho_of_uniform_column(A, t2, salt)[:, kstar - 1][ok]
    db = float(np.median(GRAV * (1.0 - ra / rb)))
    _kpp_run(A)
    zt = A.vert("zt")
    d = zt[kstar]
    ri = (d - 0.5 * EPSSFC * d) * db / (du * du)
    assert ri > RICR
    expect = zt[kstar - 1] + (zt[kstar] - zt[kstar - 1]) * np.sqrt(RICR / ri)
    hblt, kbl = A.get("HBLT")[ok], A.geti("KBL")[ok]
    err = float(np.abs(hblt - expect).max() / expect)
    assert err <= tol, "HBLT of the two-layer column differs from the closed form by %.3e (%.6f vs %.6f cm)" % (err, hblt.flat[0], expect)
    assert (kbl == kstar).all()
    return err


# ------------------------------------------------------------------------------------------------------------------
# advection of tracers (advection.F90): exact flux divergence of a linear field, monotonicity of the limited scheme
# ------------------------------------------------------------------------------------------------------------------
def _adv_setup(A, u0):
    c2dt = _prepare(A)
    _quiet(A)
    shp = A.get("UVEL", 1).shape
    for tl in range(3):
        A.set("UVEL", np.full(shp, u0), tl)
    kmt = A.geti("KMT")
    for n in range(2):
        A.set("STF", np.zeros(kmt.shape), 1, n)
    if A.cfg.vmix_choice == 3:
        for n in range(2):
            A.set("KPP_SRC", np.zeros(shp), 1, n)
    return c2dt, kmt, shp


def check_advt_linear(A, tol=1e-12):
    """Uniform zonal velocity u0 at every U point, V = 0, T = a i + b j (indices within the block), no diffusion (ah = 0):
    the east-face transport is u0 (DYU(i,j) + DYU(i,j-1)) / 2 (advection.F90:1555-1566), independent of i on the lat-lon
    grid, there is no vertical velocity, and the flux divergence is exactly  u0 a HTE_eff(j) / TAREA(j)  for the centred
    scheme (advection.F90:1667-1729) and for the third-order upwind scheme (a linear profile is interpolated exactly on a
    grid uniform in i, :2313-2676)."""
    assert A.cfg.ah == 0.0
    u0, a, b = 3.0, 2.0 ** -5, 2.0 ** -4
    c2dt, kmt, shp = _adv_setup(A, u0)
    km = A.km
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :]
    jj = np.arange(shp[-2], dtype=np.float64)[None, None, :, None]
    field = [a * ii + b * jj + np.zeros(shp), 0.5 * a * ii - 0.25 * b * jj + 1.0 + np.zeros(shp)]
    for n in range(2):
        for tl in range(3):
            A.set("TRACER", field[n], tl, n)
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    ok = _patch(kmt, km, r=4)
    dyu, tarea = A.get("DYU"), A.get("TAREA")
    ute = u0 * 0.5 * (dyu + np.roll(dyu, 1, axis=1))
    worst = 0.0
    for n, amp in ((0, a), (1, 0.5 * a)):
        expect = -(ute * amp / tarea)
        out = A.get("TRACER", 2, n) / c2dt
        for k in range(km):
            worst = max(worst, float(np.abs(out[:, k] - expect)[ok].max() / np.abs(expect)[ok].max()))
    assert worst <= tol, "advection of a linear field differs from the exact flux divergence by %.3e" % worst
    return worst


def check_lw_lim_monotone(A):
    """One-dimensional limited Lax-Wendroff advection (advection.F90:2684-3280) of a step in i by a uniform zonal flow at
    Courant number ~0.4: the advected profile X - dt div(F) has no new extremum (stays inside [lo, hi] and monotone in i across
    the step), and what the rows lose is what the flow carried across the step: sum_i TAREA div(F) = UTE (X_right - X_left)."""
    assert A.cfg.tadvect == 3 and A.cfg.ah == 0.0
    c2dt0 = 2.0 * A.scalar("dtt")
    dxt = A.get("DXT")
    u0 = 0.4 * float(np.median(dxt)) / c2dt0
    c2dt, kmt, shp = _adv_setup(A, u0)
    km = A.km
    ok = _patch(kmt, km, r=4)
    # the longest run of patch columns in a row of block 0
    b, j = 0, int(np.argmax(ok[0].sum(axis=1)))
    cols = np.flatnonzero(ok[b, j])
    runs = np.split(cols, np.flatnonzero(np.diff(cols) > 1) + 1)
    run = max(runs, key=len)
    assert len(run) >= 12
    i0, i1 = int(run[0]), int(run[-1])
    istep = (i0 + i1) // 2
    lo, hi = 2.0, 3.0
    ii = np.arange(shp[-1])[None, None, None, :]
    step = np.where(ii <= istep, lo, hi) + np.zeros(shp)
    for n, f in ((0, step), (1, 5.0 - step)):
        for tl in range(3):
            A.set("TRACER", f, tl, n)
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    dyu, tarea = A.get("DYU"), A.get("TAREA")
    ute = u0 * 0.5 * (dyu + np.roll(dyu, 1, axis=1))
    sel = slice(i0 + 2, i1 - 1)
    for n, f, jump in ((0, step, hi - lo), (1, 5.0 - step, lo - hi)):
        ft = A.get("TRACER", 2, n) / c2dt                    # = -div(F)
        for k in (0, km // 2, km - 1):
            new = (f[b, k, j] + c2dt * ft[b, k, j])[sel]
            assert new.min() >= lo - 1e-12 and new.max() <= hi + 1e-12, "limited advection created a new extremum: [%r, %r]" % (new.min(), new.max())
            d = np.diff(new) * np.sign(jump)
            assert d.min() >= -1e-12, "limited advection is not monotone across the step"
            assert np.abs(new - f[b, k, j][sel]).max() > 0.05            # the step did move
            lost = float((tarea[b, j][sel] * -ft[b, k, j][sel]).sum())
            expect = float(ute[b, j, istep] * jump)
            assert abs(lost - expect) <= 1e-11 * abs(expect), "transport across the step: %r vs %r" % (lost, expect)
    return True


# ------------------------------------------------------------------------------------------------------------------
# Gent-McWilliams / isopycnal mixing (hmix_gm.F90): a field linear in the grid indices has closed-form fluxes
# ------------------------------------------------------------------------------------------------------------------
def check_gm_linear(A, tol=2e-12):
    """T = T0 + a i + c j + b k (b < 0: stably stratified; uniform salinity; at rest), constant kappa, well below the boundary layer
    and inside the slope limits, open ocean away from coasts, on the lat-lon grid (metrics uniform in i, varying with j).
    Then the isopycnal slopes are Sx = a / (-b), Sy = c / (-b) everywhere (the expansion coefficient cancels), every taper is 1 and,
    with HYX = HTE / HUS, HXY = HTN / HUW, _w / _s the west / south neighbour's value, kappa_b = ah_bolus:
      * the east-face fluxes are equal at i and i - 1; the north-face flux is FY = dz HXY c kappa_b: dz (HXY / 4) c (4 kappa) from
        :1827-1828 (the eight-term sum holds four KAPPA_ISOP and four HOR_DIFF = 0), minus, without cancellation, the skew terms
        (HXY / 4) 4 (kappa - kappa_b) Sy dz (-b) of :1870-1896; so the horizontal part of the tendency is kappa_b c (HXY - HXY_s) / TAREA;
      * the flux through the bottom face is fz(k) = - (kappa + kappa_b) / 4 Q (dz(k) + dz(k+1)) with
        Q = Sx a (HYX + HYX_w) + Sy c (HXY + HXY_s) (:1923-2050), so the vertical part is
        (kappa + kappa_b) / 4 Q (dz(k+1) - dz(k-1)) / (dz(k) TAREA);
      * the isopycnal part added to the vertical diffusivity at the bottom of level k (:1725-1748) is
        kappa dzw(k)^2 [Sx^2 (HYX + HYX_w) + Sy^2 (HXY + HXY_s)] / (2 TAREA)  (= kappa times the squared true slope, as it should be).
    The second tracer, uniform, has no tendency at all."""
    assert A.cfg.hmix_tracer == 3 and A.cfg.vmix_choice == 1 and A.cfg.gm_transition_layer == 0
    c2dt, kmt, shp = _adv_setup(A, 0.0)
    km = A.km
    a, b, c, t0 = 2.0 ** -5, -(2.0 ** -2), 2.0 ** -6, 20.0
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :]
    jj = np.arange(shp[-2], dtype=np.float64)[None, None, :, None]
    kk = np.arange(km, dtype=np.float64)[None, :, None, None]
    field = [t0 + a * ii + c * jj + b * kk + np.zeros(shp), 0.035 + np.zeros(shp)]
    for n in range(2):
        for tl in range(3):
            A.set("TRACER", field[n], tl, n)
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    ok = _patch(kmt, km, r=4)
    kappa, Sx, Sy = A.cfg.ah, a / (-b), c / (-b)
    kappa_b = A.cfg.ah_bolus if A.cfg.ah_bolus != 0.0 else kappa
    dz, dzw = A.vert("dz"), A.vert("dzw")
    hyx, hxy = A.get("HTE") / A.get("HUS"), A.get("HTN") / A.get("HUW")
    hyx_w, hxy_s = np.roll(hyx, 1, axis=2), np.roll(hxy, 1, axis=1)
    tarea = A.get("TAREA")
    Q = Sx * a * (hyx + hyx_w) + Sy * c * (hxy + hxy_s)
    assert np.abs(hxy - hxy_s)[ok].max() > 1e-4 * hxy[ok].max()                           # ... and varying with j: the horizontal part is there
    assert np.abs(hyx - np.roll(hyx, 1, axis=2))[ok].max() <= 1e-14 * hyx[ok].max()      # the premise: metrics uniform in i
    vdc_all = A.get("VDC", 1, 0)
    vdc = vdc_all - A.cfg.const_vdc
    gt = [A.get("TRACER", 2, n) / c2dt for n in range(2)]
    dzr, dzwr = 1.0 / dz[1:km + 1], A.vert("dzwr")
    worst_g = worst_v = 0.0
    levels = list(range(4, km - 1))
    nsig = 0
    for k in levels:
        exp_v = kappa * dzw[k] * dzw[k] * (Sx * Sx * (hyx + hyx_w) + Sy * Sy * (hxy + hxy_s)) / (2.0 * tarea)
        worst_v = max(worst_v, float(np.abs(vdc[:, k] - exp_v)[ok].max() / np.abs(exp_v)[ok].max()))
        # the right-hand side also holds the explicit vertical diffusion of the old tracer with the (now larger) diffusivity
        # (vdifft, vertical_mix.F90:795-806): VDTK(k) = (VDC(k-1) (T(k-1) - T(k)) dzwr(k-1) - VDC(k) (T(k) - T(k+1)) dzwr(k)) dzr(k)
        vdtk = (vdc_all[:, k - 1] * (-b) * dzwr[k - 1] - vdc_all[:, k] * (-b) * dzwr[k]) * dzr[k - 1]
        exp_g = kappa_b * c * (hxy - hxy_s) / tarea + 0.25 * (kappa + kappa_b) * Q * (dz[k + 1] - dz[k - 1]) / (dz[k] * tarea)
        rem = gt[0][:, k - 1] - vdtk
        floor = 4.0e-16 * np.abs(vdtk)[ok].max()                                           # what the subtraction leaves of rounding
        if np.abs(exp_g)[ok].max() > 1.0e4 * floor:
            nsig += 1
            worst_g = max(worst_g, float((np.abs(rem - exp_g)[ok].max() - floor) / np.abs(exp_g)[ok].max()))
        assert np.abs(gt[1][:, k - 1])[ok].max() == 0.0
    assert nsig >= 4
    assert worst_g <= 1.0e-9, "GM tendency of a linear field differs from the closed form by %.3e" % worst_g     # what is left after the subtraction
    assert worst_v <= tol, "isopycnal part of VDC differs from its closed form by %.3e" % worst_v
    return worst_g, worst_v


def _taper_slope(control, x):
    """the slope tapers of hmix_gm.F90:1480-1594 as functions of x = SLA / slm, written from the papers the reference cites:
    'tanh' Danabasoglu & McWilliams (1995): 1/2 (1 - tanh(10 x - 4)) below x = 1, 0 above; 'notanh', its piecewise-parabolic
    stand-in: 1 up to x = 0.2, 0 from x = 0.6, in between 1/2 (1 - (2.5 x - 1)(4 - |10 x - 4|)); 'Gerd' (Gerdes et al. 1991): 1 up to
    x = 1, x^-2 above; 'clip': no taper (the slope itself is limited)."""
    x = np.asarray(x, dtype=np.float64)
    if control == 1:
        return np.where(x < 1.0, 0.5 * (1.0 - np.tanh(10.0 * x - 4.0)), 0.0)
    if control == 0:
        mid = 0.5 * (1.0 - (2.5 * x - 1.0) * (4.0 - np.abs(10.0 * x - 4.0)))
        return np.where(x <= 0.2, 1.0, np.where(x >= 0.6, 0.0, mid))
    if control == 3:
        return np.where(x > 1.0, 1.0 / (x * x), 1.0)
    return np.ones_like(x)


def check_gm_tapers(A, tol=5e-12):
    """The slope tapers of Gent-McWilliams mixing on a CONSTRUCTED slope field (until round 4 they rested on two
    restatements by one author).  T = T0 + a i + b k at rest with uniform salinity gives the isopycnal slope Sx = a / (-b) in index
    units at every quarter cell, hence the true slope magnitude of hmix_gm.F90:1431-1436

        SLA(j, k) = dzw(k) |Sx| / DXT(j) + eps

    at both half cells next to the interface below level k -- a function of latitude and depth that sweeps the break points of every
    taper.  Below the second level the near-surface taper is 1 (no KPP: the boundary layer is the first level), so with
    tau_r = taper(SLA / slm_r), tau_b = taper(SLA / slm_b) (`diff_tapering`; tau_b = tau_r when the limits are equal):

      * the isopycnal part added to the vertical diffusivity (:1725-1748) is tau_r kappa dzw(k)^2 Sx^2 (HYX + HYX_w) / (2 TAREA);
      * the stream function of the thickness diffusion at that interface, east face (:1684-1690, 2091-2097), is
        UIB(k) = tau_b kappa_b Sx HYX dzw(k), so the eddy-induced velocity of diag_gm_bolus (:2112) is
        U_ISOP(k) = (UIB(k-1) - UIB(k)) / (dz(k) HTE);
      * 'clip' limits the slope itself instead: |Sx| -> min(|Sx|, slm_r HUS / dzw(k)) (:1541-1573), both formulas with tau = 1.

    Exercised on the oracle and on the device in all four slope_control choices, with equal and with different slope limits."""
    cfg = A.cfg
    assert cfg.hmix_tracer == 3 and cfg.vmix_choice == 1 and cfg.gm_transition_layer == 0 and cfg.gm_kappa_type == 0 and cfg.gm_diag_bolus == 1
    c2dt, kmt, shp = _adv_setup(A, 0.0)
    km = A.km
    a, b, t0 = 0.5, -(2.0 ** (-12 if cfg.gm_slope_control == 3 else -10)), 2.0      # (Gerdes' taper only acts above the slope limit: steeper)
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :]
    kk = np.arange(km, dtype=np.float64)[None, :, None, None]
    field = [t0 + a * ii + b * kk + np.zeros(shp), 0.035 + np.zeros(shp)]
    for n in range(2):
        for tl in range(3):
            A.set("TRACER", field[n], tl, n)
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    ok = _patch(kmt, km, r=4)
    control = cfg.gm_slope_control
    slm_r = cfg.slm_r if cfg.slm_r != 0.0 else 0.3
    slm_b = cfg.slm_b if cfg.slm_b != 0.0 else 0.3
    kappa = cfg.ah
    kappa_b = cfg.ah_bolus if cfg.ah_bolus != 0.0 else kappa
    dz, dzw = A.vert("dz"), A.vert("dzw")
    hyx = A.get("HTE") / A.get("HUS")
    hyx_w = np.roll(hyx, 1, axis=2)
    tarea, dxt, hus, hte = A.get("TAREA"), A.get("DXT"), A.get("HUS"), A.get("HTE")
    Sx = a / (-b)
    vdc = A.get("VDC", 1, 0) - cfg.const_vdc
    uis = A.get("UISOP")

    def sx_eff(k):       # |slope| in index units after 'clip'
        return np.minimum(Sx, slm_r * hus / dzw[k]) if control == 2 else Sx + 0.0 * hus

    def sla(k):
        return dzw[k] * Sx / dxt + 1.0e-10

    seen_r, seen_b = [], []
    worst_v = worst_u = 0.0
    uib_prev, sign = None, None
    for k in range(3, km - 1):
        tr, tb = _taper_slope(control, sla(k) / slm_r), _taper_slope(control, sla(k) / slm_b)
        se = sx_eff(k)
        exp_v = tr * kappa * dzw[k] * dzw[k] * se * se * (hyx + hyx_w) / (2.0 * tarea)
        scale = (kappa * dzw[k] * dzw[k] * se * se * (hyx + hyx_w) / (2.0 * tarea))[ok].max()
        worst_v = max(worst_v, float(np.abs(vdc[:, k] - exp_v)[ok].max() / scale))
        uib = tb * kappa_b * se * hyx * dzw[k]
        if uib_prev is not None:
            exp_u = (uib_prev - uib) / (dz[k] * hte)
            got = uis[:, k - 1]
            big = np.abs(exp_u) > 1.0e-3 * np.abs(exp_u)[ok].max()
            if sign is None:     # the orientation of the slope (sign of SLX for dT/dx > 0 in stable water) is one sign for the whole field
                sel = ok & big
                sign = 1.0 if float((got[sel] * exp_u[sel]).sum()) > 0.0 else -1.0
            uscale = max(np.abs(uib_prev / (dz[k] * hte))[ok].max(), 1e-300)       # the two terms cancel partly: error relative to one of them
            worst_u = max(worst_u, float(np.abs(got - sign * exp_u)[ok].max() / uscale))
        uib_prev = uib
        seen_r.append((sla(k) / slm_r)[ok]); seen_b.append((sla(k) / slm_b)[ok])
    xr, xb = np.concatenate(seen_r), np.concatenate(seen_b)
    # the constructed field must actually visit every branch of the function under test
    if control == 0:
        for x in (xr, xb):
            assert (x < 0.2).any() and ((x > 0.25) & (x < 0.55)).any() and (x > 0.6).any(), "slopes miss a branch of the 'notanh' taper"
    elif control == 1:
        for x in (xr, xb):
            assert (x < 0.3).any() and ((x > 0.3) & (x < 0.6)).any() and (x > 1.0).any(), "slopes miss a branch of the 'tanh' taper"
    elif control == 3:
        for x in (xr, xb):
            assert (x < 1.0).any() and (x > 1.5).any(), "slopes miss a branch of Gerdes' taper"
    else:
        clipped = np.concatenate([(slm_r * hus / dzw[k] < Sx)[ok] for k in range(3, km - 1)])
        assert clipped.any() and (~clipped).any(), "slopes miss a branch of the clipping"
    assert worst_v <= tol, "tapered isopycnal part of VDC differs from its closed form by %.3e" % worst_v
    assert worst_u <= tol, "eddy-induced velocity differs from the tapered stream function's by %.3e" % worst_u
    return worst_v, worst_u


def check_gm_transition_layer(A, tol=2e-11):
    """The transition layer of Gent-McWilliams mixing (hmix_gm.F90:3183-3440 transition_layer, :3441-3743 merged_streamfunction) on the
    constructed slope field of check_gm_tapers (T = T0 + a i + b k at rest, no KPP, so the diabatic depth D is zw(1)), against what the
    two routines are supposed to deliver -- stated independently of their 250-line state machine and interpolation code:

      * INTERIOR_DEPTH I is the deepest of the grid depths zt(2), zw(2), zt(3), zw(3), ... that can be reached from zt(2) one by one
        while the isopycnal displacement over one deformation radius still reaches the diabatic layer, D >= d - R |S|(d), with
        |S| = SLA at that depth and R the Rossby radius bounded to [15, 100] km; THICKNESS = I - D.  (Closed form of SLA as in
        check_gm_tapers; the walk is the statement of Danabasoglu et al. 2008, eq. 6.)
      * the merged stream function psi(z) sampled at the half-cell centres z = zt(k) -+ dz(k) / 4 is LINEAR through the origin above D;
        in the layer it leaves that line QUADRATICALLY, psi = line - c (z - D)^2 with ONE c per column; extended to I it meets the
        first interior sample (continuity) and its slope there is the one-sided interior difference of smaller magnitude.
    Only the library's own outputs enter the second part (GM_SF_SLX, TLT_*)."""
    cfg = A.cfg
    assert cfg.hmix_tracer == 3 and cfg.vmix_choice == 1 and cfg.gm_transition_layer == 1 and cfg.gm_kappa_type == 0
    c2dt, kmt, shp = _adv_setup(A, 0.0)
    km = A.km
    a, b, t0 = 0.5, -(2.0 ** -5), 2.0          # R |S| of the order of the level depths at low latitudes, well below them at high ones
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :]
    kk = np.arange(km, dtype=np.float64)[None, :, None, None]
    field = [t0 + a * ii + b * kk + np.zeros(shp), 0.035 + np.zeros(shp)]
    for n in range(2):
        for tl in range(3):
            A.set("TRACER", field[n], tl, n)
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    ok = _patch(kmt, km, r=4)
    dz, dzw, dzwr, zt, zw = A.vert("dz"), A.vert("dzw"), A.vert("dzwr"), A.vert("zt"), A.vert("zw")
    dxt, fcort = A.get("DXT"), A.get("FCORT")
    Sx = a / (-b)
    rb = 1.0 / np.maximum(np.minimum(np.abs(fcort) / 200.0, 1.0 / 1.5e6), 1.0e-7)
    D, TH, ID = A.get("TLT_DIABATIC_DEPTH"), A.get("TLT_THICKNESS"), A.get("TLT_INTERIOR_DEPTH")
    assert np.all(D[ok] == zw[1])

    def sla(k):
        return dzw[k] * Sx / dxt + 1.0e-10

    # ---- the walk
    exp_i = np.full(D.shape, zt[2])
    going = np.ones(D.shape, dtype=bool)
    cands = [(zw[2], 2)] + [c for k in range(3, km - 1) for c in ((zt[k], k), (zw[k], k))]
    for d, k in cands:
        reach = going & (D >= d - rb * sla(k))
        exp_i = np.where(reach, d, exp_i)
        going = reach
    assert np.array_equal(ID[ok], exp_i[ok]), "INTERIOR_DEPTH differs from the walk in %d columns" % int((ID != exp_i)[ok].sum())
    assert np.array_equal(TH[ok], (exp_i - D)[ok])
    assert len(np.unique(ID[ok])) >= 4, "the constructed slopes give a trivial transition layer"
    assert not going[ok].any()
    # ---- the merged stream function, east face
    top, bot = A.get("GM_SF_SLX", 1, 0), A.get("GM_SF_SLX", 1, 1)              # (nblocks, km, ny, nx): levels 1 .. km
    zs = np.empty(2 * km); ps = np.empty((2 * km,) + D.shape)
    for k in range(1, km + 1):
        zs[2 * (k - 1)] = zt[k] - 0.25 * dz[k]; zs[2 * (k - 1) + 1] = zt[k] + 0.25 * dz[k]
        ps[2 * (k - 1)] = top[:, k - 1]; ps[2 * (k - 1) + 1] = bot[:, k - 1]
    assert zs[1] <= zw[1] < zs[2]
    slope = ps[0] / zs[0]
    scale = np.abs(ps[:, ok]).max()
    assert scale > 0.0
    worst = {"linear": float(np.abs(ps[1] - slope * zs[1])[ok].max() / scale)}
    nb, ny, nx = D.shape
    w_quad = w_cont = w_slope = 0.0
    n_quad = 0
    for bi, j, i in zip(*np.nonzero(ok)):
        d0, i0 = D[bi, j, i], ID[bi, j, i]
        p = ps[:, bi, j, i]
        inl = np.nonzero((zs > d0) & (zs <= i0))[0]
        first_int = int(np.nonzero(zs > i0)[0][0])
        if len(inl) == 0:
            continue
        cq = -(p[inl] - slope[bi, j, i] * zs[inl]) / (zs[inl] - d0) ** 2
        c0 = cq[-1]                                                      # the deepest sample carries the most signal
        if len(inl) >= 2:
            n_quad += 1
            w_quad = max(w_quad, float(np.abs((cq - c0) * (zs[inl] - d0) ** 2).max() / scale))
        T = i0 - d0
        w_cont = max(w_cont, abs(slope[bi, j, i] * i0 - c0 * T * T - p[first_int]) / scale)
        # one-sided interior differences at I: between the first and the second interior sample, and between the second and the third
        k1, h1 = first_int // 2 + 1, first_int % 2
        if h1 == 1:      # I = zt(k1): psi_I = SF(kbt, k1)
            e1 = 2.0 * dzwr[k1] * (p[first_int] - p[first_int + 1])
            e2 = 2.0 * (p[first_int + 1] - p[first_int + 2]) / dz[k1 + 1]
        else:            # I = zw(k1 - 1): psi_I = SF(ktp, k1)
            e1 = 2.0 * (p[first_int] - p[first_int + 1]) / dz[k1]
            e2 = 2.0 * dzwr[k1] * (p[first_int + 1] - p[first_int + 2])
        dpsi = e2 if abs(e2) < abs(e1) else e1
        w_slope = max(w_slope, abs((slope[bi, j, i] - 2.0 * c0 * T) + dpsi) / (scale / zw[2]))
    worst.update(quadratic=w_quad, continuity=w_cont, slope=w_slope)
    assert n_quad >= 20, "too few columns with two samples inside the transition layer"
    for what, v in worst.items():
        assert v <= tol, "merged stream function: %s violated by %.3e" % (what, v)
    return worst


def _rho_of_field(A, temp, salt):
    """in-situ density of an arbitrary (temp, salt) field: the model's own `state` phase (see _rho_of_uniform_column)"""
    keep = [(A.get("TRACER", tl, n), tl, n) for tl in range(3) for n in range(2)]
    for tl in range(3):
        A.set("TRACER", temp, tl, 0)
        A.set("TRACER", salt, tl, 1)
    A.run_phase("state")
    rho = A.get("RHO", 2)
    for arr, tl, n in keep:
        A.set("TRACER", arr, tl, n)
    return rho


def check_gm_bfre_profile(A, tol=2e-6):
    """kappa type 'bfre' (buoyancy_frequency_dependent_profile, hmix_gm.F90:3011-3180): below the surface diabatic layer the
    diffusivities are scaled by KAPPA_VERTICAL(k) = N^2(k-1) / N^2(K_MIN) bounded to [0.1, 1], N^2 at the interface below level k
    = -g (d rho / d T)(T_k, S, p_{k+1}) (T_k - T_{k+1}) / dzw(k) (uniform salinity), K_MIN the first interface below the layer.

    Constructed column: T = T(k) + a i with three linear pieces in k -- moderate, four times steeper (N^2 above the reference value:
    upper bound), then sixteen times weaker (N^2 below a tenth of it: lower bound).  The expansion coefficient comes from CENTRAL
    DIFFERENCES of the model's own density (state phase on columns of uniform temperature T_k +- delta read at level k + 1), not from
    the routine under test.  Both half cells next to an interface have the same slope a / (T_k - T_{k+1}) and the same taper, so the
    isopycnal part added to VDC there is the constant-kappa closed form of check_gm_tapers times the thickness-weighted mean
    (dz(k) KV(k) + dz(k+1) KV(k+1)) / (dz(k) + dz(k+1))."""
    cfg = A.cfg
    assert cfg.hmix_tracer == 3 and cfg.vmix_choice == 1 and cfg.gm_transition_layer == 0 and cfg.gm_kappa_type == 1 and cfg.gm_slope_control == 0
    c2dt, kmt, shp = _adv_setup(A, 0.0)
    km = A.km
    nb, _, ny, nx = shp
    a, t0, salt = 2.0 ** -6, 24.0, 0.035
    b1 = -(2.0 ** -4)
    k1, k2 = 4, 9                                               # (0-based levels) the steep piece starts at k1, the weak one at k2
    tk = np.empty(km)
    tk[0] = t0
    for k in range(1, km):
        tk[k] = tk[k - 1] + (b1 if k <= k1 else 4.0 * b1 if k <= k2 else b1 / 16.0)
    ii = np.arange(nx, dtype=np.float64)[None, None, None, :]
    T = tk[None, :, None, None] + a * ii + np.zeros(shp)
    S = salt + np.zeros(shp)
    for tl in range(3):
        A.set("TRACER", T, tl, 0); A.set("TRACER", S, tl, 1)
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    vdc = A.get("VDC", 1, 0) - cfg.const_vdc
    ok = _patch(kmt, km, r=4)
    dz, dzw = A.vert("dz"), A.vert("dzw")
    # ---- N^2 at the interfaces k = 1 .. km-1 (1-based), expansion coefficient by central differences of the model's density
    d = 2.0 ** -6
    n2 = np.zeros((km + 1,) + (nb, ny, nx))
    for k in range(1, km):                                      # interface below level k; T_k = T[:, k-1], density read at level k+1 = index k
        col = np.broadcast_to(T[:, k - 1:k], shp)
        rp, rm = _rho_of_field(A, col + d, S)[:, k], _rho_of_field(A, col - d, S)[:, k]
        n2[k] = np.maximum(0.0, -GRAV / dzw[k] * ((rp - rm) / (2.0 * d)) * (T[:, k - 1] - T[:, k]))
    kmin = 2                                                    # zw(2) is the first interface depth below the diabatic layer zw(1); N^2 > 0 there
    assert np.all(n2[kmin][ok] > 0.0)
    norm = np.ones_like(n2)
    for k in range(kmin, km):
        norm[k] = np.minimum(np.maximum(n2[k] / n2[kmin], 0.1), 1.0)
    norm[km] = norm[km - 1]
    kv = np.ones_like(n2)                                       # KAPPA_VERTICAL(k), 1-based
    for k in range(kmin + 1, km + 1):
        kv[k] = norm[k - 1]
    assert (kv[:, ok] == 0.1).any() and ((kv[:, ok] > 0.1) & (kv[:, ok] < 1.0)).any() and (kv[kmin + 2:, ok] == 1.0).any(), "the column misses a branch of the bounds"
    # ---- the isopycnal part of VDC
    kappa = cfg.ah
    slm_r = cfg.slm_r if cfg.slm_r != 0.0 else 0.3
    hyx = A.get("HTE") / A.get("HUS")
    hyx_w = np.roll(hyx, 1, axis=2)
    tarea, dxt = A.get("TAREA"), A.get("DXT")
    worst = 0.0
    for k in range(3, km - 1):
        sx = a / (tk[k - 1] - tk[k])
        tap = _taper_slope(0, (dzw[k] * sx / dxt + 1.0e-10) / slm_r)
        base = tap * kappa * dzw[k] * dzw[k] * sx * sx * (hyx + hyx_w) / (2.0 * tarea)
        mean = (dz[k] * kv[k] + dz[k + 1] * kv[k + 1]) / (dz[k] + dz[k + 1])
        worst = max(worst, float((np.abs(vdc[:, k] - base * mean) / np.abs(base))[ok].max()))
    assert worst <= tol, "isopycnal part of VDC with the N^2 profile differs from its closed form by %.3e" % worst
    return worst


def pbc_flat_grid(cfg, kstar, frac):
    """caller grid for check_kpp_hblt_two_layer_pbc: the synthetic lat-lon grid with a FLAT bottom at level kstar whose bottom cell has the
    same partial thickness frac * dz(kstar) everywhere (a record of bottom_cell_file), so that the boundary-layer depth is the same in
    every column and the horizontal filter of smooth_hblt leaves it alone"""
    from popcfg import synthetic_grid
    from orclib import Oracle
    small = type(cfg).from_buffer_copy(bytes(cfg))
    small.partial_bottom_cells = 0
    o = Oracle(small)
    dz = o.v1("dz").copy()
    o.close()
    g = synthetic_grid(cfg, stepped=False)
    g["KMT"] = np.where(g["KMT"] > 0, kstar, 0).astype(np.int32)
    g["DZBC"] = np.where(g["KMT"] > 0, frac * dz[kstar], 0.0)
    return g


def check_kpp_hblt_two_layer_pbc(A, kstar, frac, tol=2e-7):
    """check_kpp_hblt_two_layer with the velocity and density jump at the PARTIAL BOTTOM CELL itself (KBL = KMT = kstar, bottom thickness
    frac * dz; grid of pbc_flat_grid).  With partial bottom cells the reference does not use LMD94's (d - eps d / 2) db / |dV|^2 but the
    gradient form between the first T point and T point kl (vmix_kpp.F90:2359-2366, 2561-2575):
        Ri* = (db / h_T) / (|dV|^2 / h_U^2),   h_T = zt(k*-1) + (dz(k*-1) + DZT(k*) - dz(1)) / 2   (= h_U: the bottom thickness is uniform)
    and the T point of the bottom cell sits at ZKL = zt(k*-1) + (dz(k*-1) + DZT(k*)) / 2 (:2212-2220), so the root of the parabola is
        h = zt(k*-1) + (ZKL - zt(k*-1)) sqrt(Ri_c / Ri*).
    Also the non-local source (:1296-1302), which reaches the bottom cell here: its thickness-weighted column sum vanishes (the transport only
    redistributes) WITH the partial thickness -- with dz(k*) in its place it is off by the per cent the cell is thinner."""
    km = A.km
    t1, t2, salt, du = 16.0, 15.99, 0.035, 24.0        # a weak jump: Ri* ~ 0.45, so the boundary layer ends INSIDE the bottom cell, below its top face
    kmt = _kpp_setup(A, kstar, t1, t2, 1.0, -1.0e-4, u1=du, u2=0.0, salt=salt)
    # A shear of 1e-3 du across the upper layer (level 1 keeps du, so |dV|^2 at the jump is unchanged).  With NO shear above the jump the
    # bulk Richardson number there is (roundoff of the density difference of equal water) / (the eps regularisation of the denominator)
    # -- noise of either sign and of any size up to O(0.1), which the parabola takes its slope at z(k*-1) from (the reference's formula
    # has the same property; seen at km = 62, k* = 30: -0.053 at level 28 moved HBLT by 2e-4).  With it that number is O(1e-8).
    shp = A.get("UVEL", 1).shape
    lev = np.arange(1, km + 1)[None, :, None, None]
    U = np.where(lev < kstar, du * (1.0 + 1.0e-3 * (lev - 1.0) / kstar), 0.0) + np.zeros(shp)
    for tl in range(3):
        A.set("UVEL", U, tl)
    wet = kmt == kstar
    ok = wet.copy()
    for dj in range(-3, 4):
        for di in range(-3, 4):
            ok &= np.roll(np.roll(wet, dj, axis=1), di, axis=2)
    ok[:, :5, :] = False; ok[:, -5:, :] = False; ok[:, :, :5] = False; ok[:, :, -5:] = False
    assert ok.sum() > 50
    dz, zt = A.vert("dz"), A.vert("zt")
    dzbc = A.get("DZBC")
    assert np.all(np.abs(dzbc[ok] - frac * dz[kstar]) <= 1e-9 * dz[kstar])
    ra = _rho_of_uniform_column(A, t1, salt)[:, kstar - 1][ok]
    rb = _rho_of_uniform_column(A, t2, salt)[:, kstar - 1][ok]
    db = float(np.median(GRAV * (1.0 - ra / rb)))
    _kpp_run(A)
    dzb = frac * dz[kstar]
    h_t = zt[kstar - 1] + 0.5 * (dz[kstar - 1] + dzb - dz[1])
    zkl = zt[kstar - 1] + 0.5 * (dz[kstar - 1] + dzb)
    # the reference velocity is the mean over the surface layer eps zt(k*) (vmix_kpp.F90:2324-2349; full-cell depths also with partial cells)
    zw = np.concatenate([[0.0], np.cumsum(dz[1:])])
    surf = EPSSFC * zt[kstar]
    kref = next(k for k in range(1, kstar + 1) if zw[k] >= surf)
    ulev = U[0, :, 0, 0]
    uref = (ulev[kref - 1] * (surf - zw[kref - 1]) + sum(dz[k] * ulev[k - 1] for k in range(1, kref))) / surf
    ri = (db / h_t) / (uref * uref / (h_t * h_t))
    assert ri > RICR
    expect = zt[kstar - 1] + (zkl - zt[kstar - 1]) * np.sqrt(RICR / ri)
    hblt, kbl = A.get("HBLT")[ok], A.geti("KBL")[ok]
    err = float(np.abs(hblt - expect).max() / expect)
    assert (kbl == kstar).all()
    assert err <= tol, "HBLT with the jump at a partial bottom cell differs from the closed form by %.3e (%.6f vs %.6f cm)" % (err, hblt.flat[0], expect)
    full = zt[kstar - 1] + (zt[kstar] - zt[kstar - 1]) * np.sqrt(RICR / ((zt[kstar] - 0.5 * EPSSFC * zt[kstar]) * db / (du * du)))
    assert abs(full - expect) > 1.0e-3 * expect, "the case does not distinguish the partial-cell form from the full-cell one"
    # non-local source: sum_k SRC(k) DZT(k) = 0 with DZT(k*) = the partial thickness
    src = A.get("KPP_SRC", 1, 0)
    thick = np.array([dz[k] for k in range(1, kstar)] + [dzb])
    col = np.stack([src[:, k][ok] for k in range(kstar)])          # (kstar, ncol)
    s1 = np.abs((col * thick[:, None]).sum(axis=0)).max()
    s0 = (np.abs(col) * thick[:, None]).sum(axis=0).max()
    wrong = np.abs((col * np.array([dz[k] for k in range(1, kstar + 1)])[:, None]).sum(axis=0)).max()
    assert s0 > 0.0 and np.abs(col[kstar - 1]).max() > 0.0, "the non-local source does not reach the bottom cell"
    assert s1 <= 1e-13 * s0, "thickness-weighted non-local source does not sum to zero: %.3e" % (s1 / s0)
    assert wrong > 1e-4 * s0
    return err, s1 / s0


# ------------------------------------------------------------------------------------------------------------------
# the 2-D elliptic system of the barotropic mode (barotropic.F90:417-548, POP_SolversMod.F90) against tests/btrop_ref.py
# ------------------------------------------------------------------------------------------------------------------
# The cases, shared by the oracle and the device runs: the 48 x 40 "tiny" domain (1204 ocean cells; every dense or sparse reference
# solve takes well under a second).  name -> (configuration, the EVP sub-blocks the partition rule solves on this bathymetry, the
# full 8 x 8 ones among them, blocks)
BTROP_LAYOUTS = {
    "blocks-12x10": (dict(), 20, 0, 16),                                                                  # 64 sub-blocks of 6 x 5
    "one-block": (dict(block_size_x=48, block_size_y=40), 5, 5, 1),                                       # cyclic rim reads; 30 sub-blocks of 8 x 8
    "closed-stepped-24x20": (dict(block_size_x=24, block_size_y=20, ew_boundary=0, stepped_bathymetry=1), 4, 1, 4),
    "padded-28x24": (dict(block_size_x=28, block_size_y=24), 5, 5, 4),                                    # last block column / row short
    "stepped-partial-bottom-cells": (dict(stepped_bathymetry=1, partial_bottom_cells=1), 20, 0, 16),      # HU from the partial cells
}
BTROP_SOLVERS = {"pcg": 1, "chrongear": 2, "pcsi": 3}
BTROP_PRECONDITIONERS = {"diagonal": 0, "evp": 1}


def btrop_config(layout, solver="pcg", precond="diagonal", **kw):
    from popcfg import named_config
    return named_config("tiny", solver_choice=BTROP_SOLVERS[solver], precond_choice=BTROP_PRECONDITIONERS[precond], **dict(BTROP_LAYOUTS[layout][0], **kw))


def _btrop_geometry(A):
    """numbering of the ocean cells (cross-checked against get_block's global indices) and div(HU grad) assembled from grid fields"""
    import btrop_ref as br
    kmt, kmu = A.geti("KMT"), A.geti("KMU")
    blocks = A.blocks()
    idx, wet, n = br.number_cells(kmt, blocks, A.halo)
    nghost = br.check_numbering(idx, wet, blocks)
    assert nghost > 0, "no ghost cell carries an ocean cell's number: the halo update did nothing"
    G = br.assemble_div_hu_grad(idx, wet, A.get("HU"), A.get("DXU"), A.get("DYU"), kmu)
    return dict(kmt=kmt, kmu=kmu, blocks=blocks, idx=idx, wet=wet, n=n, G=G, tarea=A.get("TAREA"), dtp=A.scalar("dtp"))


def _btrop_system(A):
    """A_ref of the step just taken: div(HU grad) + the centre term in closed form, asserted symmetric and asserted to carry the
    centre term the library formed (centerWgt - centerWgtIndep)"""
    import btrop_ref as br
    S = _btrop_geometry(A)
    beta, c2dtp = br.step_parameters(A.leapfrog(), S["dtp"])
    c = br.centre_term(S["tarea"][S["wet"]], beta, c2dtp, S["dtp"])
    lib = (A.get("centerWgt") - A.get("centerWgtIndep"))[S["wet"]]
    assert np.abs(lib - c).max() <= 1e-15 * np.abs(c).max(), "centre term: %.3e of the closed form" % (np.abs(lib - c).max() / np.abs(c).max())
    S["M"], S["centre"] = br.system_matrix(S["G"], c), c
    asym = br.asymmetry(S["M"])
    assert asym <= 1e-15, "the assembled operator is not symmetric: %.3e" % asym
    return S


def _field(S, A, vec):
    """numbered vector -> halo-updated field"""
    f = np.zeros(S["wet"].shape)
    f[S["wet"]] = vec
    return A.halo(f)


def check_btrop_solve_against_direct(A, oracle=None, form=None):
    """One step (a forward step: beta = 1/2, c2dtp = dtp, centre term -2 TAREA / (dtp^2 grav)), then POP_SolversRun on a random
    right-hand side of size 1e9 on the ocean cells (solutions of a few 1e3: centimetres of sea level times grav) from a zero first
    guess, convergence_criterion = 1e-13.  Asserted on either side, with r = b - A_ref x formed by scipy from the matrix of
    tests/btrop_ref.py and x_direct its sparse direct solve:
      * return code 0 and the symmetry of A_ref, its centre term equal to the library's (_btrop_system);
      * ||r||_2 <= sqrt(convergenceCriterion) + 1e-13 ||b||_2: the solver stopped because ITS residual, summed over the same cells,
        was below that number; an operator that differs from A_ref by a relative delta leaves delta ||b||;
      * max |x - x_direct| <= ||r||_2 / min |centre term|: -A_ref = -div(HU grad) + |centre|, the first part positive semi-definite
        (check_pcsi_interval_contains_the_spectrum asserts A_ref negative definite), so ||A_ref^-1||_2 <= 1 / min |centre|;
      * on the oracle, whose nine-point operator is an entry point of its own: A x = A_ref x to 1e-14 for a random x.
    With `oracle` = what this check returned for the oracle in the same case (tests/test_gpu_btrop_pins.py): both numbers
    <= 10 x the oracle's, floored at 1e-13 (the factor covers another summation order in the reductions), and the oracle's iteration
    count.  `form`: the (solver_path, pcg_persist_used) the case must run in.

    Measured on the oracle, ||r|| / ||b|| and max |x - x_direct| / max |x_direct| (iterations): default 12 x 10 blocks pcg 7.0e-9,
    1.5e-8 (30); ChronGear 3.9e-9, 7.2e-9 (30); P-CSI 4.8e-14, 3.8e-14 (60); P-CSI + EVP 1.6e-14, 1.2e-14 (60); pcg + EVP 4.3e-9,
    6.3e-9 (30).  One 48 x 40 block: 1.0e-8, 1.5e-8 / 5.6e-9, 9.1e-9 / 4.9e-14, 5.1e-14 / 4.7e-14, 3.9e-14.  Closed 24 x 20 stepped:
    pcg 2.6e-10, 5.0e-10 (30); ChronGear 1.8e-7, 3.4e-7 (20); P-CSI 2.4e-16, 3.9e-16.  Padded 28 x 24: 9.1e-9, 1.8e-8 / 5.2e-9,
    9.5e-9 / 4.8e-14, 4.6e-14.  Stepped with partial bottom cells: pcg 2.7e-7, 5.3e-7 (20); P-CSI 2.1e-16, 4.1e-16.  The nine-point
    operator itself agrees with A_ref to 2-3e-16 on every layout; max |A_ref - A_ref^T| is exactly 0."""
    import btrop_ref as br
    A.step()
    S = _btrop_system(A)
    rng = np.random.default_rng(7)
    bv = 1.0e9 * rng.standard_normal(S["n"])
    b = _field(S, A, bv)
    rc, x, its = A.solver_run(np.zeros_like(b), b)
    assert rc == 0, "the solver did not converge"
    if form is not None:
        assert A.solver_form() == form, "the solve ran as %r, the case is about %r" % (A.solver_form(), form)
    xv = x[S["wet"]]
    xd = br.direct_solve(S["M"], bv)
    rnorm, bnorm = br.norm2(bv - S["M"] @ xv), br.norm2(bv)
    res, err = rnorm / bnorm, float(np.abs(xv - xd).max() / np.abs(xd).max())
    print("btrop solve: residual %.3e, error against the direct solve %.3e, %d iterations" % (res, err, its))
    assert rnorm <= np.sqrt(A.scalar("convergenceCriterion")) + 1e-13 * bnorm, "independent residual %.3e of the right-hand side" % res
    assert np.abs(xv - xd).max() <= rnorm / np.abs(S["centre"]).min() + 1e-13 * np.abs(xd).max(), "differs from the direct solve by %.3e" % err
    if hasattr(A, "btrop_operator"):         # where the nine-point operator is an entry point of its own: A_ref x directly
        xr = _field(S, A, rng.standard_normal(S["n"]))
        got, exp = A.btrop_operator(xr)[S["wet"]], S["M"] @ xr[S["wet"]]
        assert np.abs(got - exp).max() <= 1e-14 * np.abs(exp).max(), "the nine-point operator differs from div(HU grad) + centre by %.3e" % (np.abs(got - exp).max() / np.abs(exp).max())
    if oracle is not None:
        assert its == oracle["iterations"], "%d iterations, the oracle takes %d" % (its, oracle["iterations"])
        assert res <= max(10.0 * oracle["residual"], 1e-13), "independent residual %.3e, the oracle's is %.3e" % (res, oracle["residual"])
        assert err <= max(10.0 * oracle["error"], 1e-13), "error against the direct solve %.3e, the oracle's is %.3e" % (err, oracle["error"])
    return dict(residual=res, error=err, iterations=its)


def _fsum(a):
    """the exactly rounded sum: the summation order of the check itself must not enter a 1e-13 comparison"""
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def check_btrop_operator_properties(A, tol=1e-13):
    """operators.F90 div / grad / zcurl through the operator entry points only, at level 1 and at a level below the shallowest sill
    (where there is one: the k <= KMU / KMT masks then differ from the level-1 masks), sums over the owned cells formed exactly:
      * adjointness: sum_T psi div(u, v) = - sum_U DXU DYU (u grad_x psi + v grad_y psi) for u, v that vanish where k > KMU (div is
        area-integrated, so the U-point sum carries the area DXU DYU) -- what makes div(HU grad) symmetric;
      * sum_T div(u, v) = 0 for such a field: every U point feeds two cells with + and two with -;
      * zcurl(grad psi) = 0 on T cells whose four corner U points are ocean at that level.
    Each to `tol` = 1e-13 of the LARGEST TERM of the sum (of one term of the curl): a wrong sign or metric is O(1).
    Measured on the oracle on the five layouts, both levels: adjointness 0 .. 1.4e-15, sum of div 4e-16 .. 7e-15, curl of grad
    1.4e-16 .. 2.2e-16."""
    import btrop_ref as br
    kmt, kmu = A.geti("KMT"), A.geti("KMU")
    own = br.owned_mask(kmt.shape, A.blocks())
    dxu, dyu = A.get("DXU"), A.get("DYU")
    rng = np.random.default_rng(19)
    ksill = min(A.km, int(kmt[own & (kmt > 0)].min()) + 1)
    worst = {}
    for k in (1, ksill):
        wet_u = kmu >= k
        psi = A.halo(rng.standard_normal(kmt.shape))
        u = A.halo(np.where(wet_u & own, rng.standard_normal(kmt.shape), 0.0))
        v = A.halo(np.where(wet_u & own, rng.standard_normal(kmt.shape), 0.0))
        div = A.operator("div", k, u, v)
        gx, gy = A.operator("grad", k, psi)
        lhs_terms = (psi * div)[own]
        rhs_terms = (dxu * dyu * (u * gx + v * gy))[own]
        scale = max(np.abs(lhs_terms).max(), np.abs(rhs_terms).max())
        assert scale > 0.0 and np.abs(div[own]).max() > 0.0
        adj = abs(_fsum(lhs_terms) + _fsum(rhs_terms)) / scale
        dsum = abs(_fsum(div[own])) / np.abs(0.5 * u * dyu).max()
        curl = A.operator("zcurl", k, gx, gy)
        wet4 = np.zeros(kmt.shape, dtype=bool)
        wet4[:, 1:, 1:] = wet_u[:, 1:, 1:] & wet_u[:, :-1, 1:] & wet_u[:, 1:, :-1] & wet_u[:, :-1, :-1]
        wet4 &= own
        assert wet4.sum() > 100 and (own & (kmt >= k) & ~wet4).any()
        czero = np.abs(curl[wet4]).max() / np.abs(gx * dxu).max()
        # the masks: nothing is formed below the bottom
        assert np.all(div[own & (kmt < k)] == 0.0) and np.all(gx[own & ~wet_u] == 0.0) and np.all(gy[own & ~wet_u] == 0.0)
        print("operators at k = %d: adjointness %.2e, sum div %.2e, curl grad %.2e" % (k, adj, dsum, czero))
        assert adj <= tol, "k = %d: div and grad are not adjoint: %.3e of the largest term" % (k, adj)
        assert dsum <= tol, "k = %d: sum of div(u, v) is %.3e of the largest term" % (k, dsum)
        assert czero <= tol, "k = %d: zcurl(grad) is %.3e of a term" % (k, czero)
        worst[k] = (adj, dsum, czero)
    if A.cfg.stepped_bathymetry:
        assert ksill > 1 and ((kmu >= 1) & (kmu < ksill) & own).any(), "no sill above level %d" % ksill
    return worst


def _evp_reference(A, S):
    """the five-point operator of EVP's preprocessing (centre + four north-east weights, tests/btrop_ref.py) and the sub-blocks with
    their land flags, from grid fields and the partition rule; the north-east weight is also read off A_ref's own entries and
    compared with the library's btropWgtNE"""
    import btrop_ref as br
    wne = br.north_east_weight(A.get("HU"), A.get("DXU"), A.get("DYU"), S["kmu"])
    centre = br.five_point_centre(wne, S["kmt"], S["tarea"], S["dtp"])
    b, j, i = np.nonzero(S["wet"] & (S["kmu"] > 0))
    in_matrix = np.asarray(S["G"][S["idx"][b, j, i], S["idx"][b, j + 1, i + 1]]).reshape(-1)
    assert np.abs(in_matrix - wne[b, j, i]).max() <= 1e-15 * np.abs(wne).max()
    lib = A.get("btropWgtNE")
    own = br.owned_mask(wne.shape, S["blocks"])
    assert np.abs(lib - wne)[own].max() <= 1e-15 * np.abs(wne).max(), "btropWgtNE: %.3e" % (np.abs(lib - wne)[own].max() / np.abs(wne).max())
    return wne, centre, br.evp_subblocks(wne.shape, S["blocks"], wne)


def check_evp_is_the_local_inverse(A, min_solved, min_full=0):
    """The EVP preconditioner (preconditioner_choice = 1; POP_SolversMod.F90:2268-2369, 2434-2696) applied to a random field, before
    any step (its coefficients are those of the initial centre weight, barotropic.F90:236-238), sub-block by sub-block against
    tests/btrop_ref.py:
      * the partition and the land flags (rule of :2992-3040 and :2478-2487 restated there; on the oracle also compared with the
        tables it holds);
      * solved sub-blocks: numpy.linalg.solve of the dense five-point operator with a zero rim, to 1e-8 of the largest value of the
        sub-block -- the reference's own acceptance bound for the inverse of the influence matrix (:2594-2614);
      * land sub-blocks: r / centre (0 where the centre weight is 0), element by element to 1e-15; ghost cells 0;
      * at least `min_solved` solved sub-blocks, `min_full` of them full 8 x 8 ones: the counts follow from the bathymetry and the
        rule alone (20 of 64 with 12 x 10 blocks, 5 of 30 with one 48 x 40 block), and a run that meets only land sub-blocks fails;
      * symmetry: <y, P x> = <x, P y> to 1e-12 for positive x, y (P is the inverse of an M-matrix times -1: no cancellation).
    Measured on the oracle, worst solved sub-block: 6 x 5 sub-blocks (12 x 10 blocks) 5e-13, 1.0e-12 with partial bottom cells; full
    8 x 8 ones 1.8e-10 (one block), 2.5e-10 (closed stepped), 4.2e-10 (padded) -- the marching is ill-conditioned there; the smaller
    solved sub-blocks of the closed stepped layout 3.7e-11; land sub-blocks 3.8e-16 .. 6.0e-16; symmetry 3e-16 (12 x 10 blocks), 2e-13
    (one block), 9e-14 (padded), 9.4e-13 (closed stepped).  The 1e-12 holds with a wide margin where the sub-blocks are 6 x 5 (at most
    7e-15 over six other pairs of vectors); on the three layouts with full 8 x 8 sub-blocks it holds only just: P is the exact inverse
    to 2e-10 .. 4e-10 there and no more symmetric than that in general -- other pairs of positive vectors give 4e-14 .. 1.3e-12, pairs
    of mixed sign (standard normal) 1e-13 .. 6e-10.  That is the reference's method (its own acceptance bound is 1e-8), not a
    defect of either implementation; the vectors were fixed before these figures were taken."""
    import btrop_ref as br
    assert A.cfg.preconditioner_choice == 1
    S = _btrop_geometry(A)
    wne, centre, subs = _evp_reference(A, S)
    if hasattr(A, "evp_info"):
        xr, yr, land = A.evp_info()
        ny, nx = wne.shape[1:]
        assert xr == br.evp_partition(nx - 4) and yr == br.evp_partition(ny - 4)
        for b, j0, j1, i0, i1, ld in subs:
            assert land[(b, [y[0] for y in yr].index(j0), [x[0] for x in xr].index(i0))] == ld, (b, j0, i0)
    rng = np.random.default_rng(23)
    r = rng.standard_normal(wne.shape)
    pr = A.preconditioner(r)
    ref = br.evp_apply(centre, wne, subs, r)
    ghost = np.ones(wne.shape[1:], dtype=bool)
    ghost[2:-2, 2:-2] = False
    assert np.all(pr[:, ghost] == 0.0)
    n_solved = n_full = n_land = 0
    worst = {"solved": 0.0, "full": 0.0, "land": 0.0}
    for b, j0, j1, i0, i1, land in subs:
        got, exp = pr[b, j0:j1, i0:i1], ref[b, j0:j1, i0:i1]
        if land:
            n_land += 1
            e = float((np.abs(got - exp) / np.where(exp != 0.0, np.abs(exp), 1.0)).max())
            worst["land"] = max(worst["land"], e)
            assert e <= 1e-15, "land sub-block (%d, %d, %d): differs from r / centre by %.3e" % (b, j0, i0, e)
        else:
            full = (j1 - j0, i1 - i0) == (br.EVP_SIZE, br.EVP_SIZE)
            n_solved += 1
            n_full += int(full)
            e = float(np.abs(got - exp).max() / np.abs(exp).max())
            worst["full" if full else "solved"] = max(worst["full" if full else "solved"], e)
            assert e <= 1e-8, "sub-block (%d, %d, %d) of %d x %d cells: differs from the dense solve by %.3e" % (b, j0, i0, i1 - i0, j1 - j0, e)
    assert n_solved >= min_solved and n_full >= min_full and n_land > 0, "sub-blocks solved: %d (%d full), land: %d" % (n_solved, n_full, n_land)
    x, y = (rng.uniform(0.5, 1.5, wne.shape) for _ in range(2))
    own = br.owned_mask(wne.shape, S["blocks"])
    ypx, xpy = _fsum((y * A.preconditioner(x))[own]), _fsum((x * A.preconditioner(y))[own])
    sym = abs(ypx - xpy) / max(abs(ypx), abs(xpy))
    print("EVP: %d solved (%d full), %d land; worst %r; symmetry %.2e" % (n_solved, n_full, n_land, worst, sym))
    assert sym <= 1e-12, "the preconditioner is not symmetric: %.3e" % sym
    return dict(solved=n_solved, full=n_full, land=n_land, worst=worst, symmetry=sym)


def check_pcsi_interval_contains_the_spectrum(A):
    """Host side only (the device's PcsiMaxEigs / PcsiMinEigs are compared with the oracle's bit for bit in
    tests/test_host_grid_parity.py and tests/test_gpu_parity.py).  The Chebyshev iteration of P-CSI converges on [PcsiMinEigs,
    PcsiMaxEigs] and DIVERGES for eigenvalues of P A above PcsiMaxEigs.  Dense generalised eigensolve (scipy.linalg.eigh) of
    (-A_ref) v = lambda (-P^-1) v with A_ref of the initial centre weight (what PcsiLanczos sees) and P^-1 = the diagonal of A_ref, or,
    with the EVP preconditioner, the block-diagonal matrix of the local five-point operators of check_evp_is_the_local_inverse;
    both are asserted symmetric positive definite on the way (eigh's Cholesky factorisation of -P^-1, lambda_min > 0).
      * asserted: lambda_max <= PcsiMaxEigs, for the initial centre weight (alpha: also that of every leapfrog step) and for the
        larger one of forward steps (theta), which the solver meets with the same interval;
      * recorded, not asserted: PcsiMinEigs <= lambda_min.  It holds on NO layout: the Lanczos estimate of the low end is a Ritz value,
        which lies inside the spectrum, and the reference accepts it once it moves by less than 10 % (:2970-2976).  The price is a
        slower rate for the lowest modes, not divergence.
    Measured on the oracle, [PcsiMinEigs, PcsiMaxEigs] against the true [lambda_min, lambda_max] (leapfrog; forward): 12 x 10 blocks,
    one block and padded, diagonal [0.1775, 2.8614] / [0.1774, 2.6364]; [0.2188, 2.5537]; 12 x 10 blocks EVP [0.1893, 2.8441] /
    [0.1886, 2.6354]; closed stepped [0.2443, 2.7508] / [0.2419, 2.5589]; partial bottom cells [0.2542, 2.7246] / [0.2508, 2.5421],
    EVP [0.2585, 2.7482] / [0.2513, 2.5419].  lambda_max / PcsiMaxEigs = 0.92 .. 0.93, lambda_min / PcsiMinEigs = 0.972 .. 0.9999."""
    import btrop_ref as br
    from scipy.linalg import eigh
    assert A.cfg.solver_choice == 3
    S = _btrop_geometry(A)
    c0 = br.initial_centre_term(S["tarea"][S["wet"]], S["dtp"])
    M = br.system_matrix(S["G"], c0)
    assert br.asymmetry(M) <= 1e-15
    Ad = -M.toarray()
    if A.cfg.preconditioner_choice == 1:
        wne, centre, subs = _evp_reference(A, S)
        Pinv = -br.evp_inverse_matrix(centre, wne, subs, S["idx"], S["n"])
        assert np.abs(Pinv - Pinv.T).max() == 0.0
    else:
        Pinv = np.diag(np.diag(Ad))
    lam = eigh(Ad, Pinv, eigvals_only=True)
    assert np.linalg.eigvalsh(Ad).min() > 0.0, "A_ref is not negative definite"
    lo, hi = A.scalar("PcsiMinEigs"), A.scalar("PcsiMaxEigs")
    print("P-CSI interval [%.4f, %.4f], spectrum [%.4f, %.4f]: lambda_max / PcsiMaxEigs = %.4f, lambda_min / PcsiMinEigs = %.4f"
          % (lo, hi, lam[0], lam[-1], lam[-1] / hi, lam[0] / lo))
    assert lam[0] > 0.0
    assert lam[-1] <= hi, "the largest eigenvalue %.6f of P A lies above PcsiMaxEigs = %.6f: the Chebyshev iteration diverges" % (lam[-1], hi)
    # forward steps: the same interval, the centre term of beta = theta, c2dtp = dtp; the diagonal preconditioner follows it, EVP does not
    cf = br.centre_term(S["tarea"][S["wet"]], *br.step_parameters(0, S["dtp"]), S["dtp"])
    Af = -br.system_matrix(S["G"], cf).toarray()
    lamf = eigh(Af, Pinv if A.cfg.preconditioner_choice == 1 else np.diag(np.diag(Af)), eigvals_only=True)
    print("forward steps: spectrum [%.4f, %.4f]" % (lamf[0], lamf[-1]))
    assert lamf[0] > 0.0 and lamf[-1] <= hi, "forward steps: the largest eigenvalue %.6f lies above PcsiMaxEigs = %.6f" % (lamf[-1], hi)
    return dict(interval=(lo, hi), spectrum=(float(lam[0]), float(lam[-1])), forward=(float(lamf[0]), float(lamf[-1])))


def check_mean_sea_level_is_conserved(A, oracle=None, form=None, nsteps=12):
    """The area mean of the surface pressure, <PSURF> = sum TAREA PSURF / sum TAREA over the owned ocean cells (formed exactly), over
    12 steps of the wind-driven spin-up.  Summing the rows of A x = b - r: the columns of div(HU grad) sum to zero (sum_T div = 0,
    check_btrop_operator_properties), so sum (centre term x) = sum b - sum r with the centre term proportional to TAREA: the elliptic
    system fixes the area mean of the new pressure up to the sum of the solver's residual, and the right-hand side (a divergence,
    plus the centre term times the old pressure, no fresh-water flux) carries the old mean.  Returned: the largest |<PSURF> - <PSURF>(0)|
    and max |PSURF|.
      * P-CSI (it iterates to rounding: at least convergence_check_start = 60 iterations): drift <= 1e-12 max |PSURF|; a conservation
        error -- a centre term or an area that differs between the right-hand side and the operator -- is O(1e-3);
      * pcg / ChronGear: the drift is the solver's residual.  |sum r| <= sqrt(n) ||r||_2 < sqrt(n convergenceCriterion) per step, so
        drift <= nsteps sqrt(n convergenceCriterion) (beta c2dtp dtp grav) / sum TAREA (leapfrog values, the larger ones); with
        `oracle` (the device runs): <= 10 x the oracle's drift in the same case, as the summation order of the reductions moves the
        residual the iteration stops at.
    Measured on the oracle, in pressure units (980.6 = 1 cm of sea level; max |PSURF| = 1.7e3 .. 2.5e3, about 2 cm): P-CSI, diagonal and
    EVP, 2e-14 .. 2e-13 on every layout (1e-17 .. 1e-16 of max |PSURF|); pcg 9e-6 .. 1.7e-4 (1e-8 .. 2e-7 cm); ChronGear 1.2e-5 .. 1.4e-4,
    and 1.4e-3 / 5e-4 (diagonal / EVP) with partial bottom cells; the bound for the two is 0.098."""
    import btrop_ref as br
    S = _btrop_geometry(A)
    wet, ta = S["wet"], S["tarea"][S["wet"]]
    area = _fsum(ta)

    def mean():
        return _fsum(ta * A.get("PSURF", 1)[wet]) / area

    m0, drift, pmax, forms = mean(), 0.0, 0.0, set()
    for _ in range(nsteps):
        A.step()
        drift = max(drift, abs(mean() - m0))
        pmax = max(pmax, float(np.abs(A.get("PSURF", 1)[wet]).max()))
        forms.add(A.solver_form())
    if form is not None:
        assert forms == {form}, "the solves ran as %r, the case is about %r" % (forms, form)
    print("mean sea level: drift %.3e, max |PSURF| %.3e" % (drift, pmax))
    assert pmax > 100.0, "no sea-level signal"
    if A.cfg.solver_choice == 3:
        assert drift <= 1e-12 * pmax, "the mean surface pressure drifts by %.3e (max |PSURF| %.3e)" % (drift, pmax)
    else:
        dtp = S["dtp"]
        bound = nsteps * np.sqrt(S["n"] * A.scalar("convergenceCriterion")) * (br.ALPHA * 2.0 * dtp * dtp * br.GRAV) / area
        assert drift <= bound, "the mean surface pressure drifts by %.3e, more than the solver's residual allows (%.3e)" % (drift, bound)
        if oracle is not None:
            assert drift <= 10.0 * oracle["drift"], "the mean surface pressure drifts by %.3e, the oracle's by %.3e" % (drift, oracle["drift"])
    return dict(drift=drift, pmax=pmax)


# ------------------------------------------------------------------------------------------------------------------
# The momentum right-hand side term by term (advection.F90 advu, baroclinic.F90 clinic, hmix_del2 / hmix_del4.F90 hdiffu,
# vertical_mix.F90 vdiffu) and tracer advection (advection.F90 advt_centered / advt_upwind3 / advt_lw_lim): identities and closed
# forms that neither the reference nor either implementation evaluates in this form.
# Bounds: these are rounding-level checks.  Every docstring gives the figure the check returns on the oracle (the worst of the cases of
# tests/test_dyn_pins_oracle.py, rounded up); the oracle's bound is that figure and the device's 10 x the figure; where the figure is
# below 1e-13, both are the floor 1e-12.
# ------------------------------------------------------------------------------------------------------------------
DYN_PIN = dict(const_vvc=0.0, convect_visc=0.0, const_vdc=0.0, convect_diff=0.0, bottom_drag=0.0)    # no vertical mixing of the OLD level, no drag
GAMMA = 1.0 - 2.0 * (1.0 / 3.0)                 # time_management.F90:437-439: alpha = 1/3, gamma = 1 - 2 alpha
# configurations of the two test modules (tests/test_dyn_pins_oracle.py, tests/test_gpu_dyn_pins.py), on top of "tiny"
ONE = dict(block_size_x=48, block_size_y=40)                       # one block
STEPPED = dict(stepped_bathymetry=1)
PBC = dict(stepped_bathymetry=1, partial_bottom_cells=1)
DYN_LAYOUTS = {"one-block": ONE, "blocks-12x10": {}, "padded-28x24": dict(block_size_x=28, block_size_y=24)}
MOMENTUM = dict(am=0.0, impcor=0, **DYN_PIN)                       # advection + Coriolis alone
FRICTION = dict(impcor=0, **DYN_PIN)                               # horizontal friction alone
ADVECTION = dict(ah=0.0, **DYN_PIN)                                # tracer advection alone
DEL4 = dict(hmix_momentum=4, am=-1.0e19)
SOLID_BODY_TINY = {2: 1.29e-4, 4: 2.40e-5}                         # check_hdiffu_solid_body on the oracle, tiny: del2, del4


def _dyn_tol(A, figure):
    """the bound for a check whose oracle figure is `figure`: the floor only where the figure is below 1e-13"""
    if figure < 1.0e-13:
        return 1.0e-12
    return (10.0 if isinstance(A, GpuAdapter) else 1.0) * figure


def _sh(a, di, dj):
    """a(i + di, j + dj) (cyclic: callers read the interior only, and no stencil here is wider than the two ghost cells)"""
    return np.roll(np.roll(a, -di, axis=-1), -dj, axis=-2)


def _global_index(A):
    """global (i, j) of every cell, 1-based, ghost cells included, (nblocks, ny, nx) each: i is periodic, j is 0 outside a closed boundary"""
    bl = A.blocks()
    ig = np.stack([np.asarray(b["i_glob"]) for b in bl])[:, None, :]
    jg = np.stack([np.asarray(b["j_glob"]) for b in bl])[:, :, None]
    return ig + 0 * jg, jg + 0 * ig


def _owned(A, a):
    """the cells the blocks own (ib .. ie, jb .. je: a short last block of a padded layout owns fewer than its array holds) of a
    (nblocks, [km,] ny, nx) array, as ([km,] ncells)"""
    own = np.zeros(a.shape[:1] + a.shape[-2:], dtype=bool)
    for n, b in enumerate(A.blocks()):
        own[n, b["jb"] - 1:b["je"], b["ib"] - 1:b["ie"]] = True
    return a[own] if a.ndim == 3 else np.moveaxis(a, 1, 0)[:, own]


def _smooth_flow(A, kbot, column_balanced=False, th=None):
    """a smooth (u, v) at U points from the GLOBAL indices -- the same number in a ghost cell and in the cell it copies, periodic in
    i --, different at every level, 0 where k > kbot.  column_balanced: every column's own depth integral sum_k u(k) th(k) is zero
    (no flow through the floor of any T column, whatever the bathymetry)"""
    km = A.km
    ig, jg = _global_index(A)
    x = (2.0 * np.pi * ig / A.cfg.nx_global)[:, None]
    y = (np.pi * jg / A.cfg.ny_global)[:, None]
    lev = np.arange(1, km + 1, dtype=np.float64)[None, :, None, None]
    wet = lev <= kbot[:, None]
    if column_balanced:
        g = np.cos(np.pi * (lev - 0.5) / km) + 0.3 * np.sin(3.0 * lev) + np.zeros(wet.shape)
        depth = np.where(wet, th, 0.0).sum(axis=1)
        mean = np.where(wet, g * th, 0.0).sum(axis=1) / np.where(depth > 0.0, depth, 1.0)
        g = g - A.halo(mean)[:, None]                       # DZU of the last ghost row and column is not formed here: the owners' value
        u = (6.0 * np.cos(x + 0.4) * np.sin(y) + 3.0 * np.sin(2.0 * x) * np.cos(2.0 * y) + 2.0) * g
        v = (5.0 * np.sin(x - 0.2) * np.sin(2.0 * y) - 2.5 * np.cos(3.0 * x)) * g
    else:
        u = (6.0 * np.cos(x + 0.4) * np.sin(y) + 3.0 * np.sin(2.0 * x) * np.cos(2.0 * y) + 2.0) * np.cos(1.3 * np.pi * lev / km)
        v = (5.0 * np.sin(x - 0.2) * np.sin(2.0 * y) - 2.5 * np.cos(3.0 * x)) * (1.0 - 0.8 * np.sin(0.9 * np.pi * lev / km))
    return np.where(wet, u, 0.0), np.where(wet, v, 0.0)


def _momentum_setup(A):
    """leapfrog step parameters, no flow, flat sea surface (DHU = 0), no wind, horizontally uniform density (no pressure force, exactly:
    check_gradp), no vertical friction of the old level, no drag unless the check is about it"""
    assert A.cfg.const_vvc == 0.0 and A.cfg.convect_visc == 0.0 and A.cfg.vmix_choice == 1
    c2dt = _prepare(A)
    _quiet(A)
    km = A.km
    shp = A.get("RHO", 1).shape
    prof = 1.0 + np.round(40.0 * np.arange(km) / km) * 2.0 ** -10
    for tl in range(3):
        A.set("RHO", np.broadcast_to(prof[None, :, None, None], shp).copy(), tl)
    A.dhdt()
    return c2dt, shp


def _momentum_run(A, c2dt):
    A.run_phase("hmix_momentum")
    A.run_phase("momentum_rhs")
    return _forces(A, c2dt)


def _advu_expected(A, u, v, fv, fu):
    """-(L(u) + u v KYU - v^2 KXU) + f fv, -(L(v) + u v KXU - u^2 KYU) - f fu with L in ADVECTIVE form, on every cell (see
    check_advu_advective_form), and the share of the ocean U cells that lie above their column's bottom cell"""
    km = A.km
    dxu, dyu, uarea = (A.get(n)[:, None] for n in ("DXU", "DYU", "UAREA"))
    kxu, kyu, fcor = (A.get(n)[:, None] for n in ("KXU", "KYU", "FCOR"))
    kmu = A.geti("KMU")
    th = _thickness4(A, "U")
    ud, vd = u * dyu * th, v * dxu * th                      # transports of the U cells' own faces
    uuw = 0.25 * (ud + _sh(ud, -1, 0)) + 0.125 * (_sh(ud, 0, -1) + _sh(ud, -1, -1) + _sh(ud, 0, 1) + _sh(ud, -1, 1))
    uue = 0.25 * (_sh(ud, 1, 0) + ud) + 0.125 * (_sh(ud, 1, -1) + _sh(ud, 0, -1) + _sh(ud, 1, 1) + _sh(ud, 0, 1))
    vus = 0.25 * (vd + _sh(vd, 0, -1)) + 0.125 * (_sh(vd, -1, 0) + _sh(vd, -1, -1) + _sh(vd, 1, 0) + _sh(vd, 1, -1))
    vun = 0.25 * (_sh(vd, 0, 1) + vd) + 0.125 * (_sh(vd, -1, 1) + _sh(vd, -1, 0) + _sh(vd, 1, 1) + _sh(vd, 1, 0))
    wukb = np.cumsum((vun - vus + uue - uuw) / uarea, axis=1)                     # through the bottom face of level k, positive upwards
    wuk = np.concatenate([np.zeros_like(wukb[:, :1]), wukb[:, :-1]], axis=1)      # through its top face; 0 at the surface (DHU = 0)

    def L(al):
        up = np.concatenate([al[:, :1], al[:, :-1]], axis=1)
        dn = np.concatenate([al[:, 1:], al[:, -1:]], axis=1)
        h = (uue * (_sh(al, 1, 0) - al) + uuw * (al - _sh(al, -1, 0)) + vun * (_sh(al, 0, 1) - al) + vus * (al - _sh(al, 0, -1))) / (2.0 * uarea * th)
        z = (wuk * (up - al) + wukb * (al - dn)) / (2.0 * th)
        # level km has no bottom-face term (advection.F90:1461): what its flux form leaves is the transport through the floor times alpha
        z[:, km - 1] = (wuk * (up - al))[:, km - 1] / (2.0 * th[:, km - 1]) + (al * wukb / th)[:, km - 1]
        return h + z

    lev = np.arange(1, km + 1)[None, :, None, None]
    ocean = lev <= kmu[:, None]
    fx = np.where(ocean, -(L(u) + u * v * kyu - v * v * kxu) + fcor * fv, 0.0)
    fy = np.where(ocean, -(L(v) + u * v * kxu - u * u * kyu) - fcor * fu, 0.0)
    share = float(_owned(A, lev < kmu[:, None]).sum()) / float(_owned(A, ocean).sum())
    return fx, fy, share


def check_advu_advective_form(A):
    """advu (advection.F90:1250-1491) + Coriolis (baroclinic.F90:1758-1790) with nothing else acting (am = 0, uniform density, no vertical
    friction, no drag, DHU = 0): a smooth level-dependent (u, v) on the CURRENT level, built from the global indices, 0 below KMU.
    Transports of the U cell's faces from the 12-point averages of u DYU th, v DXU th (:1310-1336; th = dz(k), or DZU with partial
    bottom cells :1250-1300):
        div = (VUN - VUS + UUE - UUW) / UAREA,   WUKB(k) = sum_{m <= k} div(m),   WUK(k) = WUKB(k-1), WUK(1) = 0
        L(a) = [UUE (a_E - a) + UUW (a - a_W) + VUN (a_N - a) + VUS (a - a_S)] / (2 UAREA th) + [WUK (a(k-1) - a) + WUKB (a - a(k+1))] / (2 th)
        FX = -(L(u) + u v KYU - v^2 KXU) + f v',    FY = -(L(v) + u v KXU - u^2 KYU) - f u'
    L is the ADVECTIVE form; the reference and the kernels evaluate the flux form, and the two agree only if the vertical velocity
    the kernel carries down the column is the integral of the divergence of the very transports it advects with.  At k = km the
    flux form has no bottom face (:1461) and leaves a WUKB(km) / th instead of the last term.  (u', v') = (u, v) with explicit Coriolis,
    gamma (u, v) + (1 - gamma) (u, v)(old) with impcor (baroclinic.F90:1766-1769, gamma = 1/3) -- the old level then holds a DIFFERENT
    smooth field, so gamma and 1 - gamma cannot be exchanged.  Asserted on EVERY interior cell (0 on land); the cells above their
    column's bottom cell are >= 85 % of the ocean U cells.
    Oracle, largest |difference| / largest |F|: <= 4e-16 -- one 48 x 40 x 16 block flat, stepped, with partial bottom cells (the
    DZU-weighted identity holds as derived) and with impcor, 1.5e-16 .. 2.5e-16; the 12 x 10 and the padded blocks the same; 60 levels
    1.5e-16; the 'wide' grid 3.1e-16."""
    assert A.cfg.am == 0.0 and A.cfg.bottom_drag == 0.0
    c2dt, shp = _momentum_setup(A)
    kmu = A.geti("KMU")
    u, v = _smooth_flow(A, kmu)
    A.set("UVEL", u, 1)
    A.set("VVEL", v, 1)
    fu, fv = u, v
    if A.cfg.impcor:
        uo, vo = 1.0 - 1.5 * v, 0.8 * u - 2.0
        lev = np.arange(1, A.km + 1)[None, :, None, None]
        uo, vo = np.where(lev <= kmu[:, None], uo, 0.0), np.where(lev <= kmu[:, None], vo, 0.0)
        A.set("UVEL", uo, 0)
        A.set("VVEL", vo, 0)
        fu, fv = GAMMA * u + (1.0 - GAMMA) * uo, GAMMA * v + (1.0 - GAMMA) * vo
    fx, fy = _momentum_run(A, c2dt)
    ex, ey, share = _advu_expected(A, u, v, fv, fu)
    scale = max(np.abs(_owned(A, ex)).max(), np.abs(_owned(A, ey)).max())
    err = max(np.abs(_owned(A, fx - ex)).max(), np.abs(_owned(A, fy - ey)).max()) / scale
    print("advu advective form: %.3e of %.3e, %.1f %% of the ocean U cells above the bottom cell" % (err, scale, 100.0 * share))
    assert share >= 0.85
    assert (_owned(A, kmu) == 0).any() and (_owned(A, kmu) == A.km).any()
    assert err <= _dyn_tol(A, 4e-16), "advu + Coriolis differ from the advective form by %.3e" % err
    return err


def check_advu_closed_forms(A):
    """advu + explicit Coriolis on the open-ocean patch, levels above km (indices within the block), against forms that hold no sum:
      * uniform (u0, v0): L = 0, only the metric terms and f remain: FX = -(u0 v0 KYU - v0^2 KXU) + f v0, FY = -(u0 v0 KXU - u0^2 KYU) - f u0;
      * u = u0 + s i, v = 0: L(u) = u s D / UAREA with D = (2 DYU(j) + DYU(j-1) + DYU(j+1)) / 4; the divergence is the same at every level,
        so a level-independent u feels no vertical advection:  FX = -L(u), FY = u^2 KYU - f u;
      * v = v0 + t j, u = 0: L(v) = t (m(j+1) + 2 m(j) + m(j-1)) / (4 UAREA), m = v DXU:  FX = v^2 KXU + f v, FY = -L(v).
    With partial bottom cells the levels above km of a full-depth neighbourhood have whole cells: the same forms.
    Oracle: 7e-17 / 2e-16 / 3e-17 of the largest |F|."""
    assert A.cfg.am == 0.0 and A.cfg.bottom_drag == 0.0 and A.cfg.impcor == 0
    c2dt, shp = _momentum_setup(A)
    km = A.km
    ok = _patch(A.geti("KMT"), km)
    kmu = A.geti("KMU")
    assert (kmu[ok] == km).all()
    lev = np.arange(1, km + 1)[None, :, None, None]
    wet = lev <= kmu[:, None]
    dxu, dyu, uarea, kxu, kyu, fcor = (A.get(n) for n in ("DXU", "DYU", "UAREA", "KXU", "KYU", "FCOR"))
    assert np.abs(dyu - np.roll(dyu, 1, axis=2))[ok].max() <= 1e-14 * dyu[ok].max()           # the premise: metrics uniform in i
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :] + np.zeros(shp)
    jj = np.arange(shp[-2], dtype=np.float64)[None, None, :, None] + np.zeros(shp)
    u0, v0, s, t = 7.0, -4.0, 0.125, 0.25
    D = 0.25 * (2.0 * dyu + np.roll(dyu, 1, axis=1) + np.roll(dyu, -1, axis=1))
    worst = []
    for case in ("uniform", "shear-i", "shear-j"):
        u = {"uniform": u0 + 0.0 * ii, "shear-i": u0 + s * ii, "shear-j": 0.0 * ii}[case]
        v = {"uniform": v0 + 0.0 * ii, "shear-i": 0.0 * ii, "shear-j": v0 + t * jj}[case]
        A.set("UVEL", np.where(wet, u, 0.0), 1)
        A.set("VVEL", np.where(wet, v, 0.0), 1)
        fx, fy = _momentum_run(A, c2dt)
        u2, v2 = u[:, 0], v[:, 0]
        if case == "uniform":
            ex, ey = -(u2 * v2 * kyu - v2 * v2 * kxu) + fcor * v2, -(u2 * v2 * kxu - u2 * u2 * kyu) - fcor * u2
        elif case == "shear-i":
            ex, ey = -(u2 * s * D / uarea), u2 * u2 * kyu - fcor * u2
        else:
            m = v2 * dxu
            ex, ey = v2 * v2 * kxu + fcor * v2, -(t * (np.roll(m, -1, axis=1) + 2.0 * m + np.roll(m, 1, axis=1)) / (4.0 * uarea))
        scale = max(np.abs(ex)[ok].max(), np.abs(ey)[ok].max())
        e = max(max(np.abs(fx[:, k] - ex)[ok].max(), np.abs(fy[:, k] - ey)[ok].max()) for k in range(km - 1)) / scale
        print("advu closed form %s: %.3e of %.3e" % (case, e, scale))
        assert e <= _dyn_tol(A, 3e-16), "advu of the %s flow differs from the closed form by %.3e" % (case, e)
        worst.append(e)
    return max(worst)


def check_wind_stress_and_bottom_drag(A):
    """vdiffu (vertical_mix.F90:935-1010) with no viscosity: the surface level receives SMF / th(1), the bottom level of every U column
    loses bottom_drag |U_old| U_old / th(KMU) -- the OLD level, with the CURRENT one at rest here --, every other level nothing
    (th = dz, or DZU with partial bottom cells :946-995).  Oracle: 3e-16 of the largest |F|."""
    assert A.cfg.am == 0.0 and A.cfg.bottom_drag > 0.0 and A.cfg.impcor == 0
    c2dt, shp = _momentum_setup(A)
    km = A.km
    kmu = A.geti("KMU")
    ig, jg = _global_index(A)
    x, y = 2.0 * np.pi * ig / A.cfg.nx_global, np.pi * jg / A.cfg.ny_global
    smf = [0.8 * np.cos(x - 0.3) * np.sin(y) + 0.3, 0.5 * np.sin(2.0 * x) * np.sin(y) - 0.2]
    for n in range(2):
        A.set("SMF", smf[n], 1, n)
    uo, vo = _smooth_flow(A, kmu)
    A.set("UVEL", uo, 0)
    A.set("VVEL", vo, 0)
    fx, fy = _momentum_run(A, c2dt)
    th = _thickness4(A, "U")
    lev = np.arange(1, km + 1)[None, :, None, None]
    mag = A.cfg.bottom_drag * np.sqrt(uo * uo + vo * vo)
    worst = 0.0
    for f, tau, old in ((fx, smf[0], uo), (fy, smf[1], vo)):
        exp = np.where((lev == 1) & (kmu[:, None] >= 1), tau[:, None] / th, 0.0) - np.where(lev == kmu[:, None], mag * old / th, 0.0)
        worst = max(worst, np.abs(_owned(A, f - exp)).max() / np.abs(_owned(A, exp)).max())
        assert np.abs(_owned(A, np.where(lev == kmu[:, None], mag * old / th, 0.0))).max() > 1e-3 * np.abs(_owned(A, exp)).max()      # the drag is visible
    print("wind stress and bottom drag: %.3e" % worst)
    assert worst <= _dyn_tol(A, 3e-16), "wind stress / bottom drag differ from the closed form by %.3e" % worst
    return worst


def _five_point(c, a):
    """c = (centre, north, south, east, west) weights: sum over the five-point stencil of a"""
    return c[0] * a + c[1] * _sh(a, 0, 1) + c[2] * _sh(a, 0, -1) + c[3] * _sh(a, 1, 0) + c[4] * _sh(a, -1, 0)


def check_hdiffu(A):
    """Horizontal friction with nothing else acting (no flow on the current level, uniform density, explicit Coriolis, no vertical friction):
    the velocity stands on the OLD level only (the mixing level of a leapfrog step).  u = a i^2, v = 0 (i = index within the block) on
    the open-ocean patch, where the lat-lon grid's coefficients do not depend on i (DUE = DUW, DMW = -DME, asserted):
      del2 (hmix_del2.F90:892-927):  HDUK = am (2 a DUE + DUM u),   HDVK = -am (DME 4 a i + (DMC + DMN + DMS) u)
    and the mirrored field u = 0, v = a i^2:  HDUK = am (DME 4 a i + (DMC + DMN + DMS) v),  HDVK = am (2 a DUE + DUM v).
      del4 (hmix_del4.F90:730-857): the same closed forms with the d4* coefficients, times D4AMF with lvariable_hmix, are the FIRST
    Laplacian (d2u, d2v); the second one is the five-point sums of (d2u, d2v) with (DUC + DUM, DUN, DUS, DUE, DUW) and (DMC .. DMW), times am.
    Oracle, worst of both fields and components, of the largest |HD.K|: del2 9.2e-14, bound 1e-13 (u_E + u_W - 2u cancels i^2 / 2 of its
    digits); del4 1.9e-12 with 16 and with 60 levels, bound 2e-12; del4 with variable coefficients 1.91e-11, bound 2e-11 (the second
    Laplacian differences first ones that agree to 1e-3 between neighbouring rows).  None is below 1e-13, so no floor applies: the
    device's bounds are 1e-12, 2e-11 and 2e-10."""
    assert A.cfg.impcor == 0 and A.cfg.bottom_drag == 0.0
    c2dt, shp = _momentum_setup(A)
    km = A.km
    del4 = A.cfg.hmix_momentum == 4
    pre = "d4" if del4 else ""
    duc, dun, dus, due, duw, dmc, dmn, dms, dme, dmw, dum = (A.get(pre + n) for n in ("DUC", "DUN", "DUS", "DUE", "DUW", "DMC", "DMN", "DMS", "DME", "DMW", "DUM"))
    ok = _patch(A.geti("KMT"), km)
    assert np.abs(due - duw)[ok].max() <= 1e-14 * np.abs(due)[ok].max() and np.abs(dmw + dme)[ok].max() <= 1e-14 * np.abs(dme)[ok].max()
    assert np.abs(dme)[ok].max() > 0.0 and np.abs(dum)[ok].max() > 0.0
    a = 2.0 ** -6
    i2 = np.arange(shp[-1], dtype=np.float64)[None, None, :] + np.zeros(shp[:1] + shp[2:])
    q = a * i2 * i2
    lap = 2.0 * a * due + dum * q                                  # the diagonal operator on a i^2
    crs = dme * 4.0 * a * i2 + (dmc + dmn + dms) * q                # the cross operator on a i^2
    am = A.cfg.am
    amf = A.get("D4AMF") if (del4 and A.cfg.lvariable_hmix) else 1.0
    fig = (2e-11 if A.cfg.lvariable_hmix else 2e-12) if del4 else 1e-13
    worst = 0.0
    for mirrored in (False, True):
        d2u, d2v = (crs, lap) if mirrored else (lap, -crs)
        if del4:
            d2u, d2v = amf * d2u, amf * d2v
            cu, cm = (duc + dum, dun, dus, due, duw), (dmc, dmn, dms, dme, dmw)
            eu, ev = am * (_five_point(cu, d2u) + _five_point(cm, d2v)), am * (_five_point(cu, d2v) - _five_point(cm, d2u))
        else:
            eu, ev = am * d2u, am * d2v
        f3 = q[:, None] + np.zeros(shp)
        A.set("UVEL", 0.0 * f3 if mirrored else f3, 0)
        A.set("VVEL", f3 if mirrored else 0.0 * f3, 0)
        fx, fy = _momentum_run(A, c2dt)
        scale = max(np.abs(eu)[ok].max(), np.abs(ev)[ok].max())
        e = max(max(np.abs(fx[:, k] - eu)[ok].max(), np.abs(fy[:, k] - ev)[ok].max()) for k in range(km)) / scale
        assert min(np.abs(eu)[ok].max(), np.abs(ev)[ok].max()) > 1e-4 * scale                      # both components are there
        print("hdiffu %s %s: %.3e of %.3e" % ("del4" if del4 else "del2", "v = a i^2" if mirrored else "u = a i^2", e, scale))
        assert e <= _dyn_tol(A, fig), "hdiffu of a quadratic field differs from the closed form by %.3e" % e
        worst = max(worst, e)
    return worst


def check_hdiffu_solid_body(A, bound):
    """Friction of the solid-body rotation u = c cos(ULAT), v = 0 (old level): a rigid rotation is not strained, so the exact
    operator gives zero; the discrete one leaves a truncation error, |HDUK| <= bound am DUN |u| on the open-ocean patch.  A
    discretisation figure, not a rounding one: measured on the oracle 1.29e-4 on tiny (dphi = 4.5 degrees) and 2.77e-5 on twice the
    resolution (96 x 80, dphi = 2.25 degrees): O(dphi^2).  The metric term DUM cancels the five-point sum to two orders of magnitude (a
    uniform u leaves 1.1e-2), so a missing or doubled term in DUM shows as ~100 x the figure.
    del4 (hmix_momentum = 4, constant coefficients), of |am| DUN^2 |u|: 2.40e-5 on tiny, 2.46e-6 on 96 x 80; a uniform u leaves 1.9e-3.  `bound` = 2 x the oracle's figure for the grid."""
    assert A.cfg.impcor == 0 and A.cfg.bottom_drag == 0.0 and A.cfg.hmix_momentum in (2, 4) and not A.cfg.lvariable_hmix
    c2dt, shp = _momentum_setup(A)
    km = A.km
    ok = _patch(A.geti("KMT"), km)
    u2 = 10.0 * np.cos(A.get("ULAT"))
    kmu = A.geti("KMU")
    lev = np.arange(1, km + 1)[None, :, None, None]
    A.set("UVEL", np.where(lev <= kmu[:, None], u2[:, None], 0.0), 0)
    fx, fy = _momentum_run(A, c2dt)
    del4 = A.cfg.hmix_momentum == 4
    ref = abs(A.cfg.am) * A.get("d4DUN" if del4 else "DUN") ** (2 if del4 else 1) * np.abs(u2)
    fig = float(max((np.abs(fx[:, k])[ok] / ref[ok]).max() for k in range(km)))
    print("hdiffu of a solid-body rotation: %.3e of am DUN |u|" % fig)
    assert fig <= bound, "friction of a solid-body rotation: %.3e of am DUN |u| (del4: |am| DUN^2 |u|), expected <= %.3e" % (fig, bound)
    return fig


# ---- tracer advection ------------------------------------------------------------------------------------------------------
def varying_grid(cfg):
    """popcfg.synthetic_grid without steps, its cell widths varying with j as well as with i (the internal grid's are uniform in both
    index directions, so its upwind3 weights are the same numbers everywhere).  TEST DATA."""
    from popcfg import synthetic_grid
    g = synthetic_grid(cfg, stepped=False)
    row = 1.0 + 0.05 * np.cos(2.0 * np.pi * np.arange(1, cfg.ny_global + 1, dtype=np.float64) / cfg.ny_global)[:, None]
    g["HTE"], g["HUW"] = np.ascontiguousarray(g["HTE"] * row), np.ascontiguousarray(g["HUW"] * row)
    return g


def _tracer_setup(A, nsteps=2):
    """leapfrog step parameters, no flow, flat sea surface (DH = 0), no surface fluxes; advection alone: no horizontal or vertical diffusion"""
    assert A.cfg.ah == 0.0 and A.cfg.const_vdc == 0.0 and A.cfg.convect_diff == 0.0 and A.cfg.vmix_choice == 1
    c2dt = _prepare(A, nsteps)
    _quiet(A)
    kmt = A.geti("KMT")
    for n in range(A.cfg.nt):
        A.set("STF", np.zeros(kmt.shape), 1, n)
    return c2dt, kmt, A.get("TRACER", 1, 0).shape


def _tracer_run(A, c2dt):
    """-> -LTK of every tracer"""
    A.dhdt()
    A.run_phase("vmix")
    A.run_phase("hmix_tracer")
    A.run_phase("tracer_rhs")
    if A.cfg.nt > 2:
        A.run_phase("passive_rhs")
    return [A.get("TRACER", 2, n) / c2dt for n in range(A.cfg.nt)]


def _set_flow(A, u, v):
    for tl in range(3):
        A.set("UVEL", u, tl)
        A.set("VVEL", v, tl)


def check_advt_constant_and_conservation(A, nsteps=2):
    """Tracer advection (tadvect 1 centred, 2 upwind3, 3 lw_lim) with nothing else acting (ah = 0, no vertical diffusion, no fluxes,
    flat sea surface), a smooth level-dependent flow built from the global indices, every tracer of the configuration:
      (a) any such flow, tracers constant on the ocean cells and 0 on land: LTK = 0 in every cell ABOVE the bottom cell of its column
          (the bottom cell carries the flow through the floor, the reference's rule advection.F90:2110-2127).  Weights that do not sum to
          1 -- any land branch of hupw3 (:2560-2640), the boundary levels of the vertical weights (:444-488, :2399-2445) -- break it;
      (b) a flow whose depth integral sum_k u th is zero in every U column (so nothing crosses any floor), tracers 1, 3: constant, LTK = 0
          in EVERY ocean cell; tracers 0, 2: random numbers from the global indices (periodic-consistent, 0 on land):
          sum TAREA th LTK = 0 over the closed, zonally periodic domain.  Each cell forms its own east and west face value; a
          mismatch between neighbours breaks the sum.
    th = dz, or DZT / DZU with partial bottom cells.
    Oracle (of c max|u| / min DXT, and of sum |TAREA th LTK|): (a) <= 3e-16, (b) <= 4e-16 and <= 5e-18, every scheme, flat, stepped,
    partial bottom cells, 12 x 10 and padded blocks, four tracers, 16 and 60 levels, the 'wide' grid."""
    c2dt, kmt, shp = _tracer_setup(A, nsteps)
    kmu = A.geti("KMU")
    nt, km = A.cfg.nt, A.km
    lev = np.arange(1, km + 1)[None, :, None, None]
    wet = lev <= kmt[:, None]
    above = lev < kmt[:, None]
    tht, thu = _thickness4(A, "T"), _thickness4(A, "U")
    tarea, dxt = A.get("TAREA"), A.get("DXT")
    const = [2.0, 0.035, 17.0, -3.0][:nt]
    ig, jg = _global_index(A)
    G = np.random.default_rng(5).random((nt, km, A.cfg.ny_global + 1, A.cfg.nx_global + 1))
    worst = {}
    for part in ("a", "b"):
        u, v = _smooth_flow(A, kmu, column_balanced=(part == "b"), th=thu)
        _set_flow(A, u, v)
        scale = max(np.abs(u).max(), np.abs(v).max()) / _owned(A, dxt).min()
        field = [np.where(wet, c, 0.0) + np.zeros(shp) for c in const]
        if part == "b":
            for n in range(0, nt, 2):
                field[n] = np.where(wet, 1.0 + G[n][:, jg, ig].transpose(1, 0, 2, 3), 0.0)
        for n in range(nt):
            for tl in range(3):
                A.set("TRACER", field[n], tl, n)
        out = _tracer_run(A, c2dt)
        for n in range(nt):
            if part == "b" and n % 2 == 0:
                w = _owned(A, np.where(wet, tarea[:, None] * tht * out[n], 0.0))
                e = abs(_fsum(w)) / _fsum(np.abs(w))
                assert _fsum(np.abs(w)) > 0.0
                key = "conservation"
            else:
                cells = above if part == "a" else wet
                e = np.abs(_owned(A, np.where(cells, out[n], 0.0))).max() / (abs(const[n]) * scale)
                key = "constant-" + part
            worst[key] = max(worst.get(key, 0.0), float(e))
            assert e <= _dyn_tol(A, 4e-16), "tracer %d, part (%s), %s: %.3e" % (n, part, key, e)
        if part == "a":      # the flow does cross the floor somewhere: the rule is needed, and (b) is a different statement
            assert max(np.abs(_owned(A, np.where(wet & ~above, out[n], 0.0))).max() for n in range(nt)) > 1e-6 * abs(const[0]) * scale
    print("advt constant / conservation: %r" % worst)
    assert (_owned(A, kmt) == 0).any()
    return worst


def _lagrange3(x, p, f):
    """the quadratic through (p[m], f[m]), m = 0, 1, 2, at x"""
    return (f[0] * (x - p[1]) * (x - p[2]) / ((p[0] - p[1]) * (p[0] - p[2])) + f[1] * (x - p[0]) * (x - p[2]) / ((p[1] - p[0]) * (p[1] - p[2])) +
            f[2] * (x - p[0]) * (x - p[1]) / ((p[2] - p[0]) * (p[2] - p[1])))


def check_upwind3_face_values(A, direction, sign):
    """tadvect = 2: the value at a face is the quadratic through the three upstream-biased cell centres, evaluated at the face
    (advection.F90:2313-2676).  The Lagrange weights are formed here from POSITIONS -- cumulative sums of the cell widths DXT, DYT, and
    zt / zw -- not from TALFXP ... tdelzm.  ah = 0, no vertical diffusion, open-ocean patch, indices within the block.
      direction 'i' / 'j': a uniform zonal (poloidal) velocity sign * 3 at every U point, T quartic in i (j) and independent of depth.  With F_E,
        F_W the transports of the cell's faces (comp_flux_vel :2068-2127) and T* the face values -- from (i-1, i, i+1) at the east face
        of i for F > 0, from (i, i+1, i+2) for F < 0 --, and because the vertical face values of a depth-independent tracer are T itself,
            -LTK = -[F_E (T*_E - T) - F_W (T*_W - T)] / TAREA        (levels above km; the divergence of F goes into the vertical)
      direction 'k': u = s i, v = 0: the same divergence D = s HTE_eff / TAREA at every level, w(k) = D sum_{m <= k} dz(m) through the bottom
        face of level k (upwards for s > 0), T = T(z) cubic in zt: the horizontal face values are T(k), and
            LTK = T(k) D + (w(k-1) T*(k-1) - w(k) T*(k)) / dz(k),   T*(k) from (k, k+1, k+2) for upward flow, (k-1, k, k+1) for downward
        flow (:2418-2426), levels 3 .. km-3 (the boundary levels: check_advt_constant_and_conservation).
    Oracle, of the largest |LTK|: i and j, both signs, <= 9e-15 on the internal grid (16 and 60 levels) and on varying_grid, whose widths vary with i and j;
    the centred scheme differs from these forms by 5e-4.  k: 2e-14 in either direction (4e-14 with 60 levels); the centred scheme differs by 1.2e-2."""
    assert A.cfg.tadvect == 2
    c2dt, kmt, shp = _tracer_setup(A)
    km = A.km
    ok = _patch(kmt, km)
    kmu = A.geti("KMU")
    lev = np.arange(1, km + 1)[None, :, None, None]
    wetu = lev <= kmu[:, None]
    dxu, dyu, tarea = A.get("DXU"), A.get("DYU"), A.get("TAREA")
    ii = np.arange(shp[-1], dtype=np.float64)[None, None, None, :] + np.zeros(shp)
    jj = np.arange(shp[-2], dtype=np.float64)[None, None, :, None] + np.zeros(shp)
    zero = np.zeros(shp)
    if direction in ("i", "j"):
        ax = -1 if direction == "i" else -2
        w = A.get("DXT" if direction == "i" else "DYT")
        face = np.cumsum(w, axis=ax)                        # position of the east (north) face
        ctr = face - 0.5 * w
        t = ((ii if direction == "i" else jj) - 0.5 * shp[ax]) / 8.0
        T3 = 1.0 + 0.2 * t ** 4 + t ** 3 - 0.5 * t * t + 0.3 * t    # a quartic: on a uniform grid the two stencils differ by a CONSTANT for a cubic
        u0 = 3.0 * sign
        _set_flow(A, np.where(wetu, u0, 0.0) + zero if direction == "i" else zero, np.where(wetu, u0, 0.0) + zero if direction == "j" else zero)
        if direction == "i":
            F = u0 * 0.5 * (dyu + _sh(dyu, 0, -1))
            sh = lambda a, d: _sh(a, d, 0)
        else:
            F = u0 * 0.5 * (dxu + _sh(dxu, -1, 0))
            sh = lambda a, d: _sh(a, 0, d)
        T2 = T3[:, 0]
        m = (-1, 0, 1) if sign > 0 else (0, 1, 2)
        star = _lagrange3(face, [sh(ctr, d) for d in m], [sh(T2, d) for d in m])     # at the east (north) face of every cell
        expect = -(F * (star - T2) - sh(F, -1) * (sh(star, -1) - T2)) / tarea
        levels = range(km - 1)
        fig = 9e-15
    else:
        s = 0.1 * sign
        _set_flow(A, np.where(wetu, s * ii, 0.0), zero)
        assert np.abs(dyu - np.roll(dyu, 1, axis=2))[ok].max() <= 1e-14 * dyu[ok].max()
        D = s * 0.5 * (dyu + _sh(dyu, 0, -1)) / tarea
        dz, zt, zw = A.vert("dz"), A.vert("zt"), A.vert("zw")
        Tz = np.zeros(km + 3)
        zeta = zt[1:km + 1] / zt[km]
        Tz[1:km + 1] = 20.0 - 15.0 * zeta + 6.0 * zeta ** 2 - 4.0 * zeta ** 3
        T3 = Tz[1:km + 1][None, :, None, None] + zero
        depth = np.cumsum(dz[1:km + 1])
        expect = np.zeros(shp)
        for k in range(3, km - 2):                          # 1-based levels 3 .. km-3

            def star(kf):                                   # the value at the bottom face of level kf
                mm = (kf, kf + 1, kf + 2) if s > 0 else (kf - 1, kf, kf + 1)
                return _lagrange3(zw[kf], [zt[q] for q in mm], [Tz[q] for q in mm])
            expect[:, k - 1] = -(Tz[k] * D + (depth[k - 2] * D * star(k - 1) - depth[k - 1] * D * star(k)) / dz[k])
        levels = range(2, km - 3)
        fig = 4e-14
    fields = [T3, 0.5 * T3 + 0.01]
    for n in range(2):
        for tl in range(3):
            A.set("TRACER", fields[n], tl, n)
    out = _tracer_run(A, c2dt)
    if expect.ndim == 3:
        expect = expect[:, None] + zero
    worst = 0.0
    for n, fac in ((0, 1.0), (1, 0.5)):                     # the constant part of the second field is advected to nothing in either form
        got, exp = (np.moveaxis(a[:, list(levels)], 1, 0)[:, ok] for a in (out[n], fac * expect))
        worst = max(worst, float(np.abs(got - exp).max() / np.abs(exp).max()))
    print("upwind3 face values, %s, sign %+d: %.3e" % (direction, sign, worst))
    assert worst <= _dyn_tol(A, fig), "upwind3 face values (%s, sign %+d) differ from Lagrange interpolation by %.3e" % (direction, sign, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------
# KPP below the boundary layer (vmix_kpp.F90 buoydiff, ri_iwmix, ddmix, the convective term, smooth_hblt) and the equation of
# state under it, against tests/eos_ref.py (40-digit MWJF) and the closed forms of Large, McWilliams & Doney (1994).  Nothing
# below takes a density, a buoyancy difference or an expansion coefficient from the model.
# ------------------------------------------------------------------------------------------------------------------
RI_INFTY, RRHO0, DSFMAX = 0.8, 2.55, 1.0        # LMD94 (28), (31)
KPP_INTERIOR = dict(vmix_choice=3, bckgrnd_vdc2=0.0, block_size_x=48, block_size_y=40)
# the oracle's figures (tests/test_kpp_interior_pins_oracle.py prints them); the device bound is 10 x (pins._dyn_tol)
STATE_FIGURE = 9.7e-15                           # check_state_against_mpmath: below 1e-13, so the 1e-12 floor is the bound
RICHARDSON_FIGURE = {20: 5.2e-13, 60: 1.0e-12}   # check_kpp_interior_richardson by km, of kpp_rich_mix: the worst of flat, stepped, partial cells, 1-3 passes
DOUBLE_DIFFUSION_FIGURE = 1.15e-14               # check_kpp_double_diffusion, cm^2/s (km = 60; 3.0e-15 at km = 20): the floor is the bound
HBLT_SMOOTHING_FIGURE = 8.0e-12                  # check_kpp_hblt_smoothing, relative, the worst of pins.HBLT_LAYOUTS


def _density_maximum_row(pbar, salts):
    """(T, S) on the density maximum d rho / d T = 0 at pbar, by bisection of eos_ref's derivative on -2 .. 8 deg C: for every
    salinity that has one there the root and a point 1e-3 deg C to either side"""
    import eos_ref
    T, S = [], []
    for s in salts:
        f = lambda t: float(eos_ref.rho_derivs(t, s, pbar)[1])
        lo, hi = -2.0, 8.0
        if not (f(lo) > 0.0 > f(hi)):
            continue
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if f(mid) > 0.0 else (lo, mid)
        T += [lo, lo - 1.0e-3, lo + 1.0e-3]
        S += [s] * 3
    return np.array(T), np.array(S)


def check_state_against_mpmath(A, npts=200):
    """state (state_mod.F90:418-560, MWJF, 'enforce') at levels 1, km / 2, km against tests/eos_ref.py: rho relatively; d rho / d T and
    d rho / d S absolutely, scaled by the largest |derivative| of the sample (near the density maximum d rho / d T passes through zero).
    Sample: T in [-3, 32] and S in [-0.001, 0.042] (both clips hit), the exact clip values T = -2 and S = 0, and a row along the
    density maximum.  Oracle against eos_ref (km 16, 20, 60): rho 4.4e-16, d rho / d T 9.7e-15, d rho / d S 1.6e-15 (the coefficients are doubles in
    the model and decimal strings in eos_ref)."""
    import eos_ref
    km = A.km
    pz = eos_ref.pressz(km)
    rng = np.random.default_rng(7)
    worst = {"rho": 0.0, "drhodt": 0.0, "drhods": 0.0}
    for kk in (1, km // 2, km):
        Tm, Sm = _density_maximum_row(pz[kk], (0.0, 0.004, 0.008, 0.012, 0.016, 0.02))
        T = np.concatenate([rng.uniform(-3.0, 32.0, npts), [-2.0, -2.0, -2.5, 10.0, 10.0, -2.0], Tm])
        S = np.concatenate([rng.uniform(-0.001, 0.042, npts), [0.035, 0.0, 0.02, 0.0, -0.0005, -0.001], Sm])
        if kk == 1:
            assert Tm.size >= 9, "no density maximum in the sample"
        assert (T < -2.0).any() and (S < 0.0).any() and (T == -2.0).any() and (S == 0.0).any()
        r, dt, ds = eos_ref.rho_derivs(T, S, pz[kk])
        if Tm.size:
            assert dt.min() < 0.0 < dt.max()                       # the sign change of d rho / d T is inside the sample
        gr, gdt, gds = A.state(kk, T, S)
        worst["rho"] = max(worst["rho"], float(np.abs(gr / r - 1.0).max()))
        worst["drhodt"] = max(worst["drhodt"], float(np.abs(gdt - dt).max() / np.abs(dt).max()))
        worst["drhods"] = max(worst["drhods"], float(np.abs(gds - ds).max() / np.abs(ds).max()))
    print("state against 40 digits: rho %.3e, drho/dT %.3e, drho/dS %.3e" % (worst["rho"], worst["drhodt"], worst["drhods"]))
    fig = max(worst.values())
    assert fig <= _dyn_tol(A, STATE_FIGURE), "the equation of state differs from the 40-digit evaluation: %r" % worst
    return fig


def _deep_neighbourhood(kmt):
    """ocean columns of the blocks' interiors whose 3 x 3 T neighbourhood is at least as deep as themselves: the four U columns
    around them then reach their bottom, and a horizontally uniform velocity profile has a horizontally uniform shear there"""
    ok = kmt > 0
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            ok &= np.roll(np.roll(kmt, dj, axis=1), di, axis=2) >= kmt
    ok[:, :2, :] = False; ok[:, -2:, :] = False; ok[:, :, :2] = False; ok[:, :, -2:] = False
    return ok


def _set_column(A, T, S, U):
    """the same profiles T, S, (U, 0) (1-based, slot 0 unused) in every column and at every time level; no velocity below KMU"""
    km = A.km
    shp = A.get("TRACER", 1, 0).shape
    lev = np.arange(1, km + 1)[None, :, None, None]
    kmu = A.geti("KMU")[:, None]
    zero = np.zeros(shp)
    Uf = np.where(lev <= kmu, U[1:km + 1][None, :, None, None], 0.0) + zero
    for tl in range(3):
        A.set("TRACER", T[1:km + 1][None, :, None, None] + zero, tl, 0)
        A.set("TRACER", S[1:km + 1][None, :, None, None] + zero, tl, 1)
        A.set("UVEL", Uf, tl)
        A.set("VVEL", zero, tl)


def _column_db(T, S, pz, km):
    """db(k) / g = 1 - rho(T_k, S_k, p_{k+1}) / rho(T_{k+1}, S_{k+1}, p_{k+1}), k = 1 .. km-1 (buoydiff, vmix_kpp.F90:3575-3621: the upper
    water displaced to the lower level; T below -2 is raised to -2 first (:3567), which eos_ref's range rule does as well)"""
    import eos_ref
    db = np.zeros(km + 1)
    for k in range(1, km):
        db[k] = GRAV * eos_ref.one_minus_ratio(T[k], S[k], T[k + 1], S[k + 1], pz[k + 1])
    return db


CAP_JUMP, CAP_USTAR, CAP_STF = 10.0, 0.05, 5.0e-3     # levels 1, 2 warmer by 10 deg C, weak wind, stable (heating) surface flux
# one interface after the other below the cap, cyclically: the target gradient Richardson number; negative: statically unstable; None: neutral
# (three neighbours above 0.8, so that an interface stays there through three smoothing passes)
RI_CYCLE = (0.07, -0.3, 0.45, 0.76, None, 0.25, -0.6, 0.62, 1.3, 1.25, 1.2)


def _richardson_column(km, zt, pz, kcap):
    """T, S, U (1-based) of the column of check_kpp_interior_richardson.  kcap = 3: the unsheared jump between levels 2 and 3, the cycle from
    interface 3 on.  kcap = 2: no jump; a stable step of 1 deg C between levels 1 and 2 sheared to a gradient Richardson number of 0.5 -- the
    bulk Richardson number of level 2 is then 0.95 zt(2) / (zt(2) - zt(1)) times that, above critical --, the cycle from interface 2 on"""
    import eos_ref
    T, S, U = np.zeros(km + 1), np.full(km + 1, 0.035), np.zeros(km + 1)
    T[kcap] = 16.0
    T[1:kcap] = T[kcap] + (CAP_JUMP if kcap == 3 else 1.0)
    for k in range(kcap - 1 if kcap == 2 else kcap, km):
        tgt = 0.5 if k < kcap else RI_CYCLE[(k - kcap) % len(RI_CYCLE)]
        if k >= kcap:
            T[k + 1] = T[k] if tgt is None else T[k] - 1.0 if tgt > 0.0 else T[k] + 4.0   # 8 x -1 + 2 x 4 = 0 over a cycle
        if tgt is None:
            du = 3.0
        else:
            db = GRAV * float(eos_ref.one_minus_ratio(T[k], S[k], T[k + 1], S[k + 1], pz[k + 1]))
            du = np.round(64.0 * math.sqrt(abs(db) * (zt[k + 1] - zt[k]) / abs(tgt))) / 64.0
        U[k + 1] = U[k] + (du if k % 2 else -du)
    return T, S, U


def _smoothed_ri(ri, kb, km, npass):
    """the 1-2-1 smoothing of ri_iwmix (vmix_kpp.F90:1573-1603) of a column with bottom level kb: ri (1-based) holds the local values
    at k < kb; 0 at k = kb (no buoyancy difference across the floor), carried to every level below; then npass passes of 1/4, 1/2, 1/4
    with the level's own value standing in above level 1 and below level km -- none where the column has fewer than 3 levels"""
    w = np.zeros(km + 2)
    w[1:kb] = ri[1:kb]
    w[kb:km + 1] = w[kb]
    for _ in range(npass):
        if kb >= 3:
            old = w.copy()
            old[0], old[km + 1] = old[1], old[km]
            w[1:km + 1] = 0.25 * old[0:km] + 0.5 * old[1:km + 1] + 0.25 * old[2:km + 2]
    return w


def _t_to_u(A, f):
    """tgrid_to_ugrid (grid.F90): the area-weighted mean of the four T cells around a U point, 0.25 (sum of TAREA f) / UAREA"""
    ta, ua = A.get("TAREA"), A.get("UAREA")
    if f.ndim == 4:
        ta, ua = ta[:, None], ua[:, None]
    g = ta * f
    return 0.25 * (g + _sh(g, 1, 0) + _sh(g, 0, 1) + _sh(g, 1, 1)) / ua


def _profiles_to_field(table, kmt):
    """table[kb] = a profile (length n) of a column with bottom level kb -> (nblocks, n, ny, nx)"""
    return np.moveaxis(table[np.maximum(kmt, 0)], -1, 1)


def check_kpp_interior_richardson(A, kcap=3, figure=None):
    """Below the boundary layer VDC and VVC hold the interior value of ri_iwmix plus the convective term, untouched by blmix (which
    rewrites k < KBL only).  A horizontally uniform column: levels 1, 2 warmer by 10 deg C than level 3 with no shear across the jump,
    weak wind and stable forcing, which ends the boundary layer right below the jump (KBL = 3, asserted); below it one temperature step
    per interface (-1 deg C stable, +4 unstable, 0 neutral) and a zig-zag velocity with |du_k| = sqrt(|db_k| dzw_k / Ri_target_k)
    rounded to 1/64 cm/s, targets RI_CYCLE.  Expected, on every ocean column whose 3 x 3 T neighbourhood is at least as deep as itself
    and for KBL <= k < KMT:
        db_k = g (1 - rho(T_k, S_k, p_{k+1}) / rho(T_{k+1}, S_{k+1}, p_{k+1}))            buoydiff, densities of tests/eos_ref.py
        Ri_k = db_k (zt_{k+1} - zt_k) / (du_k^2 + eps)                                    vmix_kpp.F90:1564; eps = 1e-10 (:104) is the reference's
                                                                                          regularisation of the shear, written in as it is
             = db_k h / (du_k^2 + eps), h = (DZT_k + DZT_{k+1}) / 2                       partial bottom cells (:1531-1563: shear / h^2, eps / h^2)
        Ri = 0 at k = KMT, carried below; num_v_smooth_Ri passes of 1/4, 1/2, 1/4          _smoothed_ri
        nu_k = bckgrnd + kpp_rich_mix (1 - min(max(Ri_k, 0) / 0.8, 1)^2)^3                LMD94 (28)
        + convect_diff / convect_visc where db_k <= 0                                      :1218-1262: N2 > 0 is the stable case, so a neutral
                                                                                          interface is convective
    VDC(k) of both tracer classes is that; VVC(k) is tgrid_to_ugrid of the viscosity (bckgrnd_vvc = Prandtl bckgrnd_vdc) where the four
    T columns around the U point all qualify.  kcap = 2 replaces the jump by a step of 1 deg C between levels 1 and 2 sheared to Ri = 0.5
    (KBL = 2, asserted): the smoothing's rule above level 1 then reaches the asserted interfaces with moderate numbers from the second pass
    on, where the unsheared jump (Ri ~ 1e13) hides it.  Every branch must have been met: convective, Ri >= 0.8, in between, and (stepped or
    partial cells) columns shallower than km.  Returns the worst difference in units of kpp_rich_mix.  The oracle's figures: 5.2e-13 at
    km = 20 and 1.0e-12 at km = 60, the worst of flat, stepped, partial bottom cells, 1, 2, 3 passes and both caps (RICHARDSON_FIGURE).  They are the
    model's own cancellation: it forms 1 - rho_a / rho_b in float64, an absolute error of 1e-16 in a db / g of 1e-4 .. 1e-3, while
    eos_ref forms the difference in 40 digits."""
    import eos_ref
    km, cfg = A.km, A.cfg
    assert cfg.lrich == 1 and cfg.bckgrnd_vdc2 == 0.0
    kmt = _kpp_setup(A, kcap, 26.0, 16.0, CAP_USTAR, CAP_STF, salt=0.035)
    zt, dz, pz = A.vert("zt"), A.vert("dz"), eos_ref.pressz(km)
    T, S, U = _richardson_column(km, zt, pz, kcap)
    _set_column(A, T, S, U)
    _kpp_run(A)
    ok = _deep_neighbourhood(kmt)
    kbl = A.geti("KBL")
    assert (kbl[ok] == kcap).all(), "the boundary layer does not end at the cap: KBL %d .. %d" % (kbl[ok].min(), kbl[ok].max())
    KB = kcap
    db = _column_db(T, S, pz, km)
    du2 = np.zeros(km + 1)
    du2[1:km] = (U[1:km] - U[2:km + 1]) ** 2
    neutral = [k for k in range(KB, km) if T[k] == T[k + 1]]
    assert neutral and all(db[k] == 0.0 for k in neutral)
    assert all(abs(db[k]) >= 1.0e-4 * GRAV for k in range(KB, km) if k not in neutral), "a buoyancy step too small for its sign to be safe"
    dzbc = None
    if cfg.partial_bottom_cells:
        dzbc = A.get("DZBC")[ok]
        assert np.ptp(dzbc) <= 1e-9 * dzbc.max() and np.ptp(kmt[ok]) == 0          # the grid of pbc_flat_grid
        dzbc = float(dzbc.flat[0])
    vdc_t, visc_t, ri_t = np.zeros((km + 1, km + 2)), np.zeros((km + 1, km + 2)), np.zeros((km + 1, km + 2))
    bvdc, bvvc = cfg.bckgrnd_vdc1, cfg.Prandtl * cfg.bckgrnd_vdc1
    for kb in np.unique(kmt[ok]):
        h = np.zeros(km + 1)
        h[1:km] = zt[2:km + 1] - zt[1:km]
        if dzbc is not None:
            h[kb - 1] = 0.5 * (dz[kb - 1] + dzbc)
        ri = _smoothed_ri(db * h / (du2 + KPP_EPS), kb, km, cfg.num_v_smooth_Ri)
        f = (1.0 - np.minimum(np.maximum(ri, 0.0) / RI_INFTY, 1.0) ** 2) ** 3
        for k in range(KB, kb):
            conv = 1.0 if db[k] <= 0.0 else 0.0
            vdc_t[kb, k] = bvdc + cfg.kpp_rich_mix * f[k] + cfg.convect_diff * conv
            visc_t[kb, k] = bvvc + cfg.kpp_rich_mix * f[k] + cfg.convect_visc * conv
        ri_t[kb] = ri
    lev = np.arange(km + 2)[None, :, None, None]
    sel = ok[:, None] & (lev >= KB) & (lev < kmt[:, None])                       # the asserted (column, interface) pairs of VDC (levels 0 .. km+1)
    expect, ri_f = _profiles_to_field(vdc_t, kmt), _profiles_to_field(ri_t, kmt)
    worst = 0.0
    for n in range(2):
        worst = max(worst, float(np.abs(A.get("VDC", 1, n) - expect)[sel].max() / cfg.kpp_rich_mix))
    conv_f = np.broadcast_to((np.concatenate([db, [0.0]]) <= 0.0)[None, :, None, None], sel.shape)
    counts = {"convective": int((sel & conv_f).sum()), "background-only": int((sel & (ri_f >= RI_INFTY)).sum()),
              "between": int((sel & (ri_f > 0.0) & (ri_f < RI_INFTY)).sum()), "neutral": int((sel & (lev == neutral[0])).sum()),
              "columns": int(ok.sum())}
    if cfg.stepped_bathymetry or cfg.partial_bottom_cells:
        counts["shallower-than-km"] = int((sel & (kmt[:, None] < km)).sum())
    assert all(v > 0 for v in counts.values()), "a branch was not met: %r" % counts
    # VVC: U points whose four T columns all qualify, KBL <= k < KMU
    kmu = A.geti("KMU")
    oku = ok & _sh(ok, 1, 0) & _sh(ok, 0, 1) & _sh(ok, 1, 1)
    levu = np.arange(1, km + 1)[None, :, None, None]
    selu = oku[:, None] & (levu >= KB) & (levu < kmu[:, None])
    assert selu.sum() > 0
    expu = _t_to_u(A, _profiles_to_field(visc_t, kmt)[:, 1:km + 1])
    worst_u = float(np.abs(A.get("VVC") - expu)[selu].max() / cfg.kpp_rich_mix)
    print("KPP interior (smoothing passes %d): VDC %.3e, VVC %.3e of kpp_rich_mix; %r" % (cfg.num_v_smooth_Ri, worst, worst_u, counts))
    fig = max(worst, worst_u)
    assert fig <= _dyn_tol(A, RICHARDSON_FIGURE[km] if figure is None else figure), "interior KPP coefficients differ from the closed forms by %.3e of kpp_rich_mix (VDC %.3e, VVC %.3e)" % (fig, worst, worst_u)
    return fig


# double diffusion: one interface after the other below the cap, cyclically.  ("finger" | "dc", R_rho), the two quadrants without a term, and a step
# of temperature alone; the two last-but-one entries also bring salinity and temperature back to where the cycle began
DD_CYCLE = (("finger", 1.16), ("finger", 1.5), ("finger", 1.95), ("finger", 3.0), ("finger", 4.0), ("dc", 0.03), ("dc", 0.2), ("dc", 0.3),
            ("dc", 0.55), ("dc", 0.6), ("ds0", None), ("stable", None), ("unstable", None))
DD_DENSITY_STEP = 1.2e-4                          # |alpha dT - beta dS| of every constructed step: |db| stays above 1e-4 g


def _dd_terms(T, S, pz, km):
    """alpha dT and beta dS of every interface (ddmix, vmix_kpp.F90:3404-3445): the expansion coefficients are the means of the two
    levels', each at its OWN pressure, from tests/eos_ref.py"""
    import eos_ref
    _, rt, rs = eos_ref.rho_derivs(T[1:km + 1], S[1:km + 1], pz[1:km + 1])
    adt, bds = np.zeros(km + 1), np.zeros(km + 1)
    adt[1:km] = -0.5 * (rt[:-1] + rt[1:]) * (T[1:km] - T[2:km + 1])
    bds[1:km] = 0.5 * (rs[:-1] + rs[1:]) * (S[1:km] - S[2:km + 1])
    return adt, bds


def _double_diffusion_column(km, pz):
    """T, S (1-based) of the column of check_kpp_double_diffusion: the steps are sized with eos_ref's coefficients (the expected values
    are formed from the column as it stands, whatever the steps turn out to be) and rounded to 2^-20 deg C and 2^-30 g/g"""
    import eos_ref
    T0, S0 = 20.0, 0.035
    T, S = np.zeros(km + 1), np.zeros(km + 1)
    T[3], S[3] = T0, S0
    T[1] = T[2] = T0 + CAP_JUMP
    S[1] = S[2] = S0
    d = DD_DENSITY_STEP
    for k in range(3, km):
        kind, R = DD_CYCLE[(k - 3) % len(DD_CYCLE)]
        _, rtk, rsk = (float(x) for x in eos_ref.rho_derivs(T[k], S[k], pz[k]))
        rt, rs = rtk, rsk
        for _ in range(4):                         # the coefficients are the means of the two levels': settle the lower level's
            if kind == "finger":                   # alpha dT > beta dS > 0
                b = d / (R - 1.0); a = R * b
            elif kind == "dc":                     # beta dS < alpha dT < 0
                b = -d / (1.0 - R); a = R * b
            elif kind == "ds0":
                a, b = 2.0e-4, 0.0
            elif kind == "stable":                 # warm and fresh over cold and salty: salinity back to S0 + 2e-4
                a, b = 2.0e-4, rs * (S[k] - (S0 + 2.0e-4))
            else:                                  # cold and salty over warm and fresh: temperature back to T0; statically unstable
                a, b = -rt * (T[k] - T0), rs * 2.0e-4
            T[k + 1] = np.round((T[k] + a / rt) * 2.0 ** 20) / 2.0 ** 20      # alpha dT = -rho_T (T_k - T_{k+1})
            S[k + 1] = np.round((S[k] - b / rs) * 2.0 ** 30) / 2.0 ** 30      # beta dS = rho_S (S_k - S_{k+1})
            _, rtn, rsn = (float(x) for x in eos_ref.rho_derivs(T[k + 1], S[k + 1], pz[k + 1]))
            rt, rs = 0.5 * (rtk + rtn), 0.5 * (rsk + rsn)
    return T, S


def check_kpp_double_diffusion(A, figure=DOUBLE_DIFFUSION_FIGURE):
    """ddmix (vmix_kpp.F90:3404-3497) with lrich = 0 and no velocity: below the boundary layer (the cap of check_kpp_interior_richardson)
    VDC of the temperature class (n = 0) and of the salinity class (n = 1) hold the background, the double-diffusive term and the
    convective term.  With alpha dT = -1/2 (rho_T(k at p_k) + rho_T(k+1 at p_{k+1})) (T_k - T_{k+1}), beta dS = 1/2 (rho_S ...) (S_k - S_{k+1})
    (derivatives of tests/eos_ref.py) and R = alpha dT / beta dS:
      salt fingering, alpha dT > beta dS > 0:    nu_S = 1.0 (1 - (min(R, 2.55) - 1) / 1.55)^3,  nu_T = 0.7 nu_S
      diffusive convection, beta dS < alpha dT < 0:  nu_T = 1.5e-2 * 0.909 exp(4.6 exp(-0.54 (1 / R - 1))),
                                                 nu_S = nu_T (1.85 - 0.85 / R) R for R > 0.5, else 0.15 R nu_T          LMD94 (32)-(34)
    LMD94 (31) has the bracket of the fingering form SQUARED before the cube, (1 - ((R - 1) / (R0 - 1))^2)^3; the reference has no square
    (vmix_kpp.F90:3468-3469) and this check follows the reference.  The column (DD_CYCLE) holds fingering at R = 1.16, 1.5, 1.95 and at
    3 and 4 (beyond Rrho0 = 2.55: no mixing), diffusive convection at 0.03, 0.2, 0.3, 0.55 and 0.6 (both sides of the 0.5 switch), one interface in
    each of the two quadrants without a term (one of them statically unstable) and one with dS = 0; every |db| is above 1e-4 g and every R
    at least 0.02 from 1, 0.5 and 2.55.  The count of interfaces per branch is asserted, and VDC n = 0 differs from n = 1 wherever a term acts.
    Returns the worst difference in cm^2/s (dsfmax = 1); the oracle's figures are 3.0e-15 (km = 20) and 1.15e-14 (km = 60), flat and stepped."""
    import eos_ref
    km, cfg = A.km, A.cfg
    assert cfg.ldbl_diff == 1 and cfg.lrich == 0 and cfg.bckgrnd_vdc2 == 0.0
    kmt = _kpp_setup(A, 3, 30.0, 20.0, CAP_USTAR, CAP_STF, salt=0.035)
    pz = eos_ref.pressz(km)
    T, S = _double_diffusion_column(km, pz)
    _set_column(A, T, S, np.zeros(km + 1))
    _kpp_run(A)
    ok = _deep_neighbourhood(kmt)
    kbl = A.geti("KBL")
    assert (kbl[ok] == 3).all(), "the boundary layer does not end below the cap: KBL %d .. %d" % (kbl[ok].min(), kbl[ok].max())
    KB = 3
    db = _column_db(T, S, pz, km)
    adt, bds = _dd_terms(T, S, pz, km)
    assert all(abs(db[k]) >= 1.0e-4 * GRAV for k in range(KB, km))
    nu = np.zeros((2, km + 2))                       # [class, interface]
    branch = {}
    for k in range(KB, km):
        a, b = adt[k], bds[k]
        R = a / b if b != 0.0 else np.inf
        if a > b > 0.0:
            assert min(abs(R - 1.0), abs(R - RRHO0)) >= 0.02
            nus = DSFMAX * (1.0 - (min(R, RRHO0) - 1.0) / (RRHO0 - 1.0)) ** 3
            nu[0, k], nu[1, k] = 0.7 * nus, nus
            branch[k] = "fingering" if R < RRHO0 else "fingering-beyond-Rrho0"
        elif b < a < 0.0:
            assert min(abs(R - 1.0), abs(R - 0.5), R) >= 0.02
            nut = 1.5e-2 * 0.909 * math.exp(4.6 * math.exp(-0.54 * (1.0 / R - 1.0)))
            nu[0, k], nu[1, k] = nut, nut * ((1.85 - 0.85 / R) * R if R > 0.5 else 0.15 * R)
            branch[k] = "diffusive-R>0.5" if R > 0.5 else "diffusive-R<=0.5"
        else:
            branch[k] = "dS=0" if b == 0.0 else "warm-fresh-over-cold-salty" if (a > 0.0 and b < 0.0) else \
                "cold-salty-over-warm-fresh" if (a < 0.0 and b > 0.0) else "unstable-same-sign"
        conv = cfg.convect_diff if db[k] <= 0.0 else 0.0
        nu[:, k] += cfg.bckgrnd_vdc1 + conv
    assert "unstable-same-sign" not in branch.values()
    lev = np.arange(km + 2)[None, :, None, None]
    sel = ok[:, None] & (lev >= KB) & (lev < kmt[:, None])
    names = np.array([branch.get(k, "") for k in range(km + 2)])
    counts = {b: int((sel & (names == b)[None, :, None, None]).sum()) for b in
              ("fingering", "fingering-beyond-Rrho0", "diffusive-R>0.5", "diffusive-R<=0.5", "dS=0", "warm-fresh-over-cold-salty", "cold-salty-over-warm-fresh")}
    counts["convective"] = int((sel & (np.concatenate([db, [1.0]]) <= 0.0)[None, :, None, None]).sum())
    counts["columns"] = int(ok.sum())
    if cfg.stepped_bathymetry:
        counts["shallower-than-km"] = int((sel & (kmt[:, None] < km)).sum())
    assert all(v > 0 for v in counts.values()), "a branch was not met: %r" % counts
    got = [A.get("VDC", 1, n) for n in range(2)]
    worst = 0.0
    for n in range(2):
        worst = max(worst, float(np.abs(got[n] - nu[n][None, :, None, None])[sel].max() / DSFMAX))
    acts = sel & (nu[0] != nu[1])[None, :, None, None]
    assert acts.sum() > 0 and (got[0][acts] != got[1][acts]).all() and np.array_equal(got[0][sel & ~acts], got[1][sel & ~acts])
    print("KPP double diffusion: %.3e cm^2/s; %r" % (worst, counts))
    assert worst <= _dyn_tol(A, figure), "double-diffusive coefficients differ from the closed forms by %.3e cm^2/s" % worst
    return worst


# name -> (configuration, k*, asserted columns with a land neighbour required, whether the bottom clamp acts on an asserted column)
HBLT_LAYOUTS = {
    "one-block": (dict(block_size_x=48, block_size_y=40), 8, 10, False),
    "blocks-12x10": (dict(), 8, 10, False),                                                     # the neighbours come through the halo
    "closed-stepped-24x20": (dict(block_size_x=24, block_size_y=20, ew_boundary=0, stepped_bathymetry=1), 8, 10, False),
    "closed-stepped-24x20-jump-below-shallow-columns": (dict(block_size_x=24, block_size_y=20, ew_boundary=0, stepped_bathymetry=1), 14, 10, True),
}


def check_kpp_hblt_smoothing(A, kstar,figure=HBLT_SMOOTHING_FIGURE, min_land=10):
    """smooth_hblt (vmix_kpp.F90:3797-3870) on the two-layer column of check_kpp_hblt_two_layer with a lower-layer temperature that varies
    with the global (i, j): the unsmoothed depth of a column with KMT >= k* is its own closed form,
        h(i, j) = zt(k*-1) + (zt(k*) - zt(k*-1)) sqrt(Ri_c / Ri*(i, j)),   Ri* = (d - eps d / 2) db(i, j) / |dV|^2,  d = zt(k*),
    with db from tests/eos_ref.py, and zt(KMT) for a column that ends above the jump (no level exceeds Ri_c).  Expected HBLT: the 5-point
    mean with weights 1/2 and 1/8, a land neighbour's weight moved to the centre, clamped at zt(KMT) and floored at zt(1); expected KBL:
    the level with zt(k-1) < HBLT <= zt(k), at least 2.  Asserted on the ocean columns whose ocean neighbours are all deeper than k*;
    at least min_land of them have a land neighbour, and some have none.  Returns the worst relative difference and the counts.  The
    oracle's figure is 7.9e-12 on every layout of HBLT_LAYOUTS (what the closed form leaves out of the bulk Richardson number's denominator: the unresolved shear of the
    neutral lower layer and eps."""
    import eos_ref
    km = A.km
    t1, salt, du = 16.0, 0.035, 14.0
    kmt = _kpp_setup(A, kstar, t1, 15.0, 1.0, -1.0e-4, u1=du, u2=0.0, salt=salt)
    ig, jg = _global_index(A)
    t2 = 15.0 - 0.4 * (1.0 + np.sin(2.0 * np.pi * ig / A.cfg.nx_global + 0.3) * np.cos(3.0 * np.pi * jg / A.cfg.ny_global))     # 14.2 .. 15
    t2 = np.round(t2 * 64.0) / 64.0                                                                                              # few distinct values
    shp = A.get("TRACER", 1, 0).shape
    lev = np.arange(1, km + 1)[None, :, None, None]
    Tf = np.where(lev < kstar, t1, t2[:, None]) + np.zeros(shp)
    Uf = np.where((lev < kstar) & (lev <= A.geti("KMU")[:, None]), du, 0.0) + np.zeros(shp)
    for tl in range(3):
        A.set("TRACER", Tf, tl, 0)
        A.set("UVEL", Uf, tl)
    _kpp_run(A)
    zt = A.vert("zt")
    pz = eos_ref.pressz(km)
    db = GRAV * eos_ref.one_minus_ratio(t1, salt, t2, salt, pz[kstar])
    d = zt[kstar]
    ri = (d - 0.5 * EPSSFC * d) * db / (du * du)
    assert ri.min() > RICR
    ocean = kmt > 0
    h0 = np.where(kmt >= kstar, zt[kstar - 1] + (zt[kstar] - zt[kstar - 1]) * np.sqrt(RICR / ri), zt[np.maximum(kmt, 0)])
    cc = np.full(kmt.shape, 0.5)
    hs = np.zeros(kmt.shape)
    nland = np.zeros(kmt.shape, dtype=int)
    deep = np.ones(kmt.shape, dtype=bool)
    for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        on, hn = _sh(ocean, di, dj), _sh(h0, di, dj)
        cc = cc + np.where(on, 0.0, 0.125)
        hs = hs + np.where(on, 0.125 * hn, 0.0)
        nland += ~on
        deep &= ~on | (_sh(kmt, di, dj) > kstar)
    hs = hs + cc * h0
    expect = np.maximum(np.minimum(hs, zt[np.maximum(kmt, 0)]), zt[1])
    ok = ocean & deep
    ok[:, :2, :] = False; ok[:, -2:, :] = False; ok[:, :, :2] = False; ok[:, :, -2:] = False
    ok = ok & _owned_mask(A)
    counts = {"columns": int(ok.sum()), "land-neighbour": int((ok & (nland > 0)).sum()), "no-land-neighbour": int((ok & (nland == 0)).sum()),
              "clamped-at-the-bottom": int((ok & (hs > zt[np.maximum(kmt, 0)])).sum())}
    hblt, kbl = A.get("HBLT"), A.geti("KBL")
    err = float((np.abs(hblt - expect) / expect)[ok].max())
    kexp = np.maximum(np.searchsorted(zt[1:km + 1], expect, side="left") + 1, 2)
    edge = np.abs(expect[..., None] - zt[1:km + 1]).min(axis=-1) <= 1.0e-5 * expect          # a depth this close to a level's is not asked for its level
    print("smooth_hblt: %.3e; %r" % (err, counts))
    assert counts["land-neighbour"] >= min_land and counts["no-land-neighbour"] > 0, counts
    assert err <= _dyn_tol(A, figure), "smoothed HBLT differs from the closed form by %.3e" % err
    assert (kbl == kexp)[ok & ~edge].all()
    return err, counts


def _owned_mask(A):
    own = np.zeros(A.geti("KMT").shape, dtype=bool)
    for n, b in enumerate(A.blocks()):
        own[n, b["jb"] - 1:b["je"], b["ib"] - 1:b["ie"]] = True
    return own
