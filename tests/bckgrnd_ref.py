"""NumPy restatement of the lhoriz_varying_bckgrnd branch of init_vmix_kpp (vmix_kpp.F90:551-602): the latitude-varying KPP background
diffusivity from TLAT and TLON, with one boolean mask per branch of the reference's statements.

Arrays have any one shape; TLAT and TLON are in radians, as the model holds them.  bckgrnd_vvc = Prandtl * field; the reference copies
level 1 of both to every level (:606-609)."""
import numpy as np

RADIAN = 180.0 / (4.0 * np.arctan(1.0))
CESM = dict(bckgrnd_vdc_eq=0.01, bckgrnd_vdc_psim=0.13, bckgrnd_vdc_ban=1.0)      # with bckgrnd_vdc1 = 0.16 (gx3v7, gx1v6, gx1v7)
MASKS = ("south", "band", "north", "banda_north", "banda_middle", "banda_south", "arctic")


def field(TLAT, TLON, bckgrnd_vdc1, bckgrnd_vdc_eq=0.01, bckgrnd_vdc_psim=0.13, bckgrnd_vdc_ban=1.0, larctic_bckgrnd_vdc=False):
    """(bckgrnd_vdc, masks): masks[name] is where the branch `name` of MASKS is taken (the Arctic one is empty without
    larctic_bckgrnd_vdc); a later branch overwrites an earlier one, as the statements follow each other"""
    lat, lon = np.asarray(TLAT) * RADIAN, np.asarray(TLON) * RADIAN       # TLATD, TLOND
    psis = bckgrnd_vdc_psim * np.exp(-(0.4 * (lat + 28.9)) ** 2)
    psin = bckgrnd_vdc_psim * np.exp(-(0.4 * (lat - 28.9)) ** 2)
    b = bckgrnd_vdc_eq + psin + psis
    m = {"south": lat < -10.0, "band": (lat >= -10.0) & (lat <= 10.0), "north": lat > 10.0}
    b = np.where(m["band"], b + bckgrnd_vdc1 * (lat / 10.0) ** 2, b + bckgrnd_vdc1)
    m["banda_north"] = (lat < -1.0) & (lat > -4.0) & (lon > 103.0) & (lon < 134.0)
    m["banda_middle"] = (lat <= -4.0) & (lat > -7.0) & (lon > 106.0) & (lon < 140.0)
    m["banda_south"] = (lat <= -7.0) & (lat > -8.3) & (lon > 111.0) & (lon < 142.0)
    for n in ("banda_north", "banda_middle", "banda_south"):
        b = np.where(m[n], bckgrnd_vdc_ban, b)
    m["arctic"] = (lat >= 70.0) if larctic_bckgrnd_vdc else np.zeros(lat.shape, dtype=bool)
    b = np.where(m["arctic"], bckgrnd_vdc_eq, b)
    return b, m


def from_nml(TLAT, TLON, bckgrnd_vdc1, nml):
    """field() for a pop_kpp_bckgrnd_nml (the ctypes mirror PopKppBckgrndNml)"""
    return field(TLAT, TLON, bckgrnd_vdc1, nml.bckgrnd_vdc_eq, nml.bckgrnd_vdc_psim, nml.bckgrnd_vdc_ban, bool(nml.larctic_bckgrnd_vdc))


def tlon(ULAT, ULON, first_row=None):
    """calc_tpoints (grid.F90:2985-3100) for longitude, block by block: the angle of the Cartesian average of the four surrounding U
    points, 0 <= TLON < 2 pi.  ULAT, ULON: (nblocks, ny_block, nx_block); the result is formed at i, j >= 1 (0 elsewhere), which covers
    the physical cells.  first_row[b]: the 0-based row of block b that is row 1 of the domain (or None): it copies the row north of it."""
    x, y = np.cos(ULON) * np.cos(ULAT), np.sin(ULON) * np.cos(ULAT)
    avg = lambda a: 0.25 * (a[:, 1:, 1:] + a[:, :-1, 1:] + a[:, 1:, :-1] + a[:, :-1, :-1])
    out = np.zeros(ULAT.shape)
    out[:, 1:, 1:] = np.arctan2(avg(y), avg(x))
    for b, j in enumerate(first_row if first_row is not None else []):
        if j is not None:
            out[b, j] = out[b, j + 1]
    return np.where(out < 0.0, out + 2.0 * np.pi, out)
