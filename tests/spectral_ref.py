"""numpy restatement of the dispersion model of zoic_amd/csrc/spectral.hpp (shared by tests/test_spectral_cpu.py and
tests/test_spectral_gpu.py): every operation in float32 with one rounding, B in float64 rounded once."""
import numpy as np

LAMBDA_D = np.float32(587.5618)
LAMBDA_D32 = LAMBDA_D      # the name the modules use that also hold an f64 LAMBDA_D
LAMBDA_F, LAMBDA_C = 486.1327, 656.2725
# the eight fixed wavelengths of the spectral tests: both ends of the range, the F, d and C lines among them
WAVES = np.array([360.0, 420.0, 486.1327, 530.0, LAMBDA_D, 610.0, 656.2725, 830.0], np.float32)
# wavelengths every spectral call rejects
BAD = np.array([np.nan, np.inf, -np.inf, 0.0, -500.0, 359.9, 830.1], np.float32)
SINGLET = """# singlet, V = 30
50.0\t6.0\t1.5168\t30.0\t20.0
-50.0\t2.0\t0.0\t0.0\t20.0
0.0\t45.0\t0.0\t0.0\t18.0
"""


def cauchy_b(ior_d, abbe):
    """B_i per medium: (n_d - 1) / (V (1/lF^2 - 1/lC^2)) in float64, rounded once; 0 for air, V <= 0 or V not finite"""
    ior_d = np.asarray(ior_d, np.float32)
    abbe = np.asarray(abbe, np.float32)
    out = np.zeros(ior_d.shape, np.float32)
    span = 1.0 / (LAMBDA_F * LAMBDA_F) - 1.0 / (LAMBDA_C * LAMBDA_C)
    for i in range(ior_d.size):
        if ior_d[i] != np.float32(1.0) and np.isfinite(abbe[i]) and abbe[i] > 0:
            out[i] = np.float32(np.float64(ior_d[i] - np.float32(1.0)) / (np.float64(abbe[i]) * span))
    return out


def dl(lam):
    lam = np.float32(lam)
    inv_d2 = np.float32(1.0) / (LAMBDA_D * LAMBDA_D)
    return np.float32(np.float32(1.0) / (lam * lam) - inv_d2)


def spectral_iors(ior_d, b, lam):
    """n_i(lambda) = n_d + (B dl): a float32 multiply, then a float32 add"""
    ior_d = np.asarray(ior_d, np.float32)
    b = np.asarray(b, np.float32)
    return (ior_d + (b * dl(lam)).astype(np.float32)).astype(np.float32)


def interface_terms(ior_d, b, lam):
    """per interface of the trace: (ior1, ior2, eta, tirPossible) as the reference's rules give them (zoic.cpp:1013, 1019)"""
    n = spectral_iors(ior_d, b, lam)
    ior2 = np.append(n[1:], np.float32(1.0)).astype(np.float32)
    eta = np.where(ior2 == np.float32(1.0), n, (n / ior2).astype(np.float32)).astype(np.float32)
    return n, ior2, eta, n > ior2
