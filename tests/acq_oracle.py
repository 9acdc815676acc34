"""Arbitrary-precision expected improvement (mpmath, 80 digits) for the per-query tail tests of EI / PI / UCB.

EI(mu, sd, t) = sd * (phi(g) - g * Q(g)),  g = (t - mu) / sd,  Q(g) = 1 - Phi(g) = erfc(g / sqrt 2) / 2.
Q is taken from erfc: written as `1 - ncdf(g)` the reference itself cancels (at 60 digits it is wrong from g = 17 on).
Inputs are taken exactly (`mpf(float(x))`): an fp32 value is not re-rounded, and the g of the reference is the exact quotient
of the numbers handed in, so the reference carries no rounding of its own that a bound would have to pay for."""
import mpmath as mp
import numpy as np

DPS = 80
GAMMAS = (-10.0, -3.0, 0.0, 2.0, 4.0, 5.0, 6.0, 7.0, 8.0, 8.5, 10.0, 20.0, 37.0)
C_HOST = 4.0     # measured in test_acq_host.py::test_stable_form_constant (worst ratio 3.45 at gamma = 1.31)
EPS64 = 2.0**-52
EPS32 = 2.0**-24


def exact_ei_gamma(gamma):
  """EI / sd at gamma (an mpf)."""
  with mp.workdps(DPS):
    g = mp.mpf(float(gamma))
    return mp.npdf(g) - g * mp.erfc(g / mp.sqrt(2)) / 2


def exact_ei(mu, sd, target):
  """EI of the exact numbers mu, sd, target (an mpf)."""
  with mp.workdps(DPS):
    mu, sd, target = mp.mpf(float(mu)), mp.mpf(float(sd)), mp.mpf(float(target))
    g = (target - mu) / sd
    return sd * (mp.npdf(g) - g * mp.erfc(g / mp.sqrt(2)) / 2)


def exact_gamma(mu, sd, target):
  with mp.workdps(DPS):
    return float((mp.mpf(float(target)) - mp.mpf(float(mu))) / mp.mpf(float(sd)))


def exact_cdf(u):
  """Phi(u) through erfc: relative accuracy in the lower tail."""
  with mp.workdps(DPS):
    return mp.erfc(-mp.mpf(float(u)) / mp.sqrt(2)) / 2


def rel_to(value, exact):
  """|value - exact| / |exact| as a float (exact: mpf, non-zero)."""
  with mp.workdps(DPS):
    return float(abs(mp.mpf(float(value)) - exact) / abs(exact))


def log_sensitivity(gamma):
  """|d ln EI / d ln gamma| = |gamma Q(gamma) / (phi - gamma Q)| (mpmath); the bounds use gamma**2 + 2 >= this."""
  with mp.workdps(DPS):
    g = mp.mpf(float(gamma))
    q = mp.erfc(g / mp.sqrt(2)) / 2
    return float(abs(g * q / (mp.npdf(g) - g * q)))


def fp64_bound(gamma):
  """Relative bound of an fp64 evaluation of phi(u) + u Phi(u) at u = -gamma, host libm (C_HOST measured on the CPU)."""
  return C_HOST * (1.0 + float(gamma)**4) * EPS64


def ei_array(mu, sd, target):
  """exact_ei over arrays, rounded to fp64 (relative error 2**-53: use only where that is far below the bound)."""
  mu, sd = np.asarray(mu), np.asarray(sd)
  return np.array([float(exact_ei(m, s, target)) for m, s in zip(mu.ravel(), sd.ravel())]).reshape(mu.shape)
