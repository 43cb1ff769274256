"""
Hardening curves of the fifth material model ('vmi': von Mises with isotropic hardening on a piecewise-linear curve,
include/fep.h, fep_return_map_vmi_*), built on the host.  The kernels take breakpoints `kappa` (kappa[0] = 0, increasing) and
one slope dR/dkappa per segment, the last segment running to infinity; kappa is the sum of the plastic multipliers and R the
growth of the yield radius Y = sqrt(2/3) sigma_y, so a uniaxial table (eps_p_bar, sigma_y) maps with
    kappa = sqrt(3/2) eps_p_bar,      R = sqrt(2/3) (sigma_y - sigma_y0).
No transcendental function reaches the device: a Voce curve is sampled into segments here.
"""
import numpy as np

MAX_SEGMENTS = 8                                            # FEP_MAX_HARDENING_SEGMENTS


def check_curve(kappa, slope, shear=None, a=None, Y=None):
    """-> (kappa, slope) as float64 arrays, or ValueError: 1 .. 8 segments, kappa[0] == 0, strictly increasing, everything
    finite (what fep_ctx_set_hardening refuses with FEP_EINVAL), and, where `shear`, `a` and `Y` are given as numbers or
    arrays, the law's preconditions 2G + a + slope[j] > 0 at every point and Y + R > 0 at every breakpoint (a falling last
    segment leaves the radius positive only up to some kappa, which is the caller's to stay below)."""
    kappa = np.array(kappa, dtype=np.float64).ravel()
    slope = np.array(slope, dtype=np.float64).ravel()
    if kappa.size != slope.size or not 1 <= kappa.size <= MAX_SEGMENTS:
        raise ValueError(f'a hardening curve has 1 .. {MAX_SEGMENTS} segments, one breakpoint and one slope each; '
                         f'got {kappa.size} and {slope.size}')
    if not (np.isfinite(kappa).all() and np.isfinite(slope).all()):
        raise ValueError('hardening curve: kappa and slope must be finite')
    if kappa[0] != 0 or not (np.diff(kappa) > 0).all():
        raise ValueError('hardening curve: kappa[0] must be 0 and kappa strictly increasing')
    if shear is not None and a is not None:
        H0 = float(np.min(2 * np.asarray(shear, dtype=np.float64) + np.asarray(a, dtype=np.float64)))
        if not H0 + slope.min() > 0:
            raise ValueError(f'hardening curve: 2G + a + slope must stay positive, got {H0:g} + {slope.min():g}')
    if Y is not None:
        Y0 = float(np.min(np.asarray(Y, dtype=np.float64)))
        if not Y0 + curve_radius(kappa, slope).min() > 0:
            raise ValueError('hardening curve: the yield radius Y + R must stay positive at every breakpoint')
    return kappa, slope


def curve_radius(kappa, slope):
    """R at the breakpoints as the library forms it: R[0] = 0, R[j+1] = R[j] + slope[j] * (kappa[j+1] - kappa[j])."""
    R = np.zeros(len(kappa))
    for j in range(1, len(kappa)):
        R[j] = R[j - 1] + slope[j - 1] * (kappa[j] - kappa[j - 1])
    return R


def hardening_curve(eps_p_bar, sigma_y):
    """A uniaxial table, yield stress `sigma_y` against equivalent plastic strain `eps_p_bar` (eps_p_bar[0] = 0, increasing,
    at most 8 rows), as the model takes it: -> (Y, kappa, slope) with Y = sqrt(2/3) sigma_y[0] the initial yield radius, one
    segment per row, the stress interpolated linearly between the rows and constant behind the last (slope 0)."""
    eps = np.array(eps_p_bar, dtype=np.float64).ravel()
    sig = np.array(sigma_y, dtype=np.float64).ravel()
    if eps.size != sig.size or eps.size < 1:
        raise ValueError('hardening_curve: one yield stress per plastic strain')
    if not sig[0] > 0:
        raise ValueError('hardening_curve: the initial yield stress must be positive')
    kappa = np.sqrt(1.5) * eps
    R = np.sqrt(2 / 3) * (sig - sig[0])
    slope = np.zeros(eps.size)
    if eps.size > 1:
        with np.errstate(divide='ignore', invalid='ignore'):
            slope[:-1] = np.diff(R) / np.diff(kappa)
    kappa, slope = check_curve(kappa, slope)
    return float(np.sqrt(2 / 3) * sig[0]), kappa, slope


def voce_curve(sigma_0, sigma_inf, b, n_seg=MAX_SEGMENTS, eps_max=None):
    """The saturating curve sigma_y = sigma_0 + (sigma_inf - sigma_0) (1 - exp(-b eps_p_bar)) sampled into `n_seg` segments
    (2 .. 8): -> (Y, kappa, slope) as hardening_curve, the last slope 0.  The n_seg rows lie at equal steps of the saturated
    fraction 1 - exp(-b eps) between 0 and its value at `eps_max` (default: where 99 % of the growth is reached, ln(100) / b),
    so the chords are shortest where the curve bends most."""
    n_seg = int(n_seg)
    if not 2 <= n_seg <= MAX_SEGMENTS:
        raise ValueError(f'voce_curve: n_seg in 2 .. {MAX_SEGMENTS}')
    if not (b > 0 and sigma_0 > 0 and np.isfinite(sigma_inf)):
        raise ValueError('voce_curve: b > 0, sigma_0 > 0, sigma_inf finite')
    eps_max = np.log(100.0) / b if eps_max is None else float(eps_max)
    if not eps_max > 0:
        raise ValueError('voce_curve: eps_max > 0')
    frac = np.arange(n_seg) / (n_seg - 1) * (1 - np.exp(-b * eps_max))
    eps = -np.log1p(-frac) / b
    eps[-1] = eps_max
    return hardening_curve(eps, sigma_0 + (sigma_inf - sigma_0) * frac)
