"""Inputs and the yardstick of the corotating paired-XOR tests (tests/test_gpu_paired_xor.py, tests/test_paired_xor_host.py).

The yardstick is the oracle's existing pieces composed here, each pinned against the reference's own statements by the g17 and
mode-operator goldens: convert_to_conjugate_pairs -> truncate -> + 0.0 -> xor_timeseries one way (scri/SpEC/file_io/
corotating_paired_xor.py:70-90), xor_timeseries_reverse -> convert_from_conjugate_pairs the way back (:240,255)."""
import functools

import numpy as np

from oracle import utilities_ref, waveform_modes_ref
from oracle.containers import WM, Corotating, h

FIXED_SHAPES = [(2, 2, 1), (2, 2, 2), (2, 3, 257), (2, 8, 700), (0, 16, 513), (0, 24, 65)]
TOLERANCES = [1e-10, 1e-3]
MARGIN = 1e-9  # every row's -log2(norm tol / sqrt(n_modes)) lies at least this far from an integer


def n_modes(ell_min, ell_max):
    return (ell_max + 1) ** 2 - ell_min**2


@functools.lru_cache(maxsize=None)
def smooth_modes(ell_min, ell_max, n, seed=20240229):
    """Seeded modes [n, n_modes], smooth in time: per mode a rotating phasor, a slow sinusoid and a constant under a decaying envelope.
    Returned read-only (the cases share it)."""
    rng = np.random.default_rng(seed + 1000 * ell_min + 10 * ell_max + n)
    nm = n_modes(ell_min, ell_max)
    t = np.linspace(0.0, 10.0, n) if n > 1 else np.zeros(1)
    a = rng.normal(size=(3, nm)) + 1j * rng.normal(size=(3, nm))
    omega = rng.uniform(0.5, 3.0, size=nm)
    data = (a[0] * np.exp(1j * np.outer(t, omega)) + 0.1 * a[1] * np.sin(t)[:, None] + a[2]) * np.exp(-0.05 * t)[:, None]
    data = np.ascontiguousarray(data)
    data.setflags(write=False)
    t.setflags(write=False)
    return t, data


def container(t, data, ell_min, ell_max):
    return WM(t=np.array(t), data=np.array(data), ell_min=ell_min, ell_max=ell_max, dataType=h, frameType=Corotating)


def oracle_paired(data, ell_min, ell_max):
    return waveform_modes_ref.convert_to_conjugate_pairs(container(np.zeros(data.shape[0]), data, ell_min, ell_max)).data


def oracle_pack(data, ell_min, ell_max, tol):
    """uint64 [n, 2 n_modes]: the reference's packed modes"""
    w = container(np.zeros(data.shape[0]), data, ell_min, ell_max)
    w = waveform_modes_ref.truncate(waveform_modes_ref.convert_to_conjugate_pairs(w), tol=tol)
    packed = w.data + 0.0
    return np.ascontiguousarray(utilities_ref.xor_timeseries(packed)).view(np.uint64)


def oracle_xor_real(x):
    """uint64 words of a real series (time, log frame): + 0.0, then xor_timeseries"""
    x = np.array(x, dtype=float) + 0.0
    return np.ascontiguousarray(utilities_ref.xor_timeseries(x)).view(np.uint64)


def oracle_unpack(words, ell_min, ell_max):
    """complex [n, n_modes] from uint64 [n, 2 n_modes]"""
    data = np.ascontiguousarray(utilities_ref.xor_timeseries_reverse(np.array(words, dtype=np.uint64))).view(np.complex128)
    return waveform_modes_ref.convert_from_conjugate_pairs(container(np.zeros(data.shape[0]), data, ell_min, ell_max)).data


def exponent_margin(data, ell_min, ell_max, tol):
    """smallest distance over the rows of -log2(norm tol / sqrt(n_modes)) from an integer (norm of the paired row, as truncate sees it)"""
    paired = oracle_paired(data, ell_min, ell_max)
    x = -np.log2(np.linalg.norm(paired, axis=1) * (tol / np.sqrt(paired.shape[1])))
    return float(np.min(np.abs(x - np.round(x))))


def restated_pack(data, ell_min, ell_max, tol):
    """The arithmetic of the pack kernel restated in numpy, operation for operation: (a + conj b) times the double 1/sqrt2, the norm summed
    column by column, the exponent read with frexp, the scale built with ldexp, rint, the sign-bit test, the XOR."""
    n, nm = data.shape
    r = 1.0 / np.sqrt(2.0)
    paired = np.array(data)
    for ell in range(ell_min, ell_max + 1):
        for m in range(1, ell + 1):
            ip, im = ell * (ell + 1) - ell_min**2 + m, ell * (ell + 1) - ell_min**2 - m
            a, b = data[:, ip], data[:, im]
            paired[:, ip] = ((a.real + b.real) * r) + 1j * ((a.imag - b.imag) * r)
            paired[:, im] = ((a.real - b.real) * r) + 1j * ((a.imag + b.imag) * r)
    total = np.zeros(n)
    for j in range(nm):
        total += paired[:, j].real * paired[:, j].real + paired[:, j].imag * paired[:, j].imag
    f, k = np.frexp(np.sqrt(total) * (tol / np.sqrt(nm)))
    e = np.where(f == 0.5, 1 - k, -k)
    v = np.rint(np.ascontiguousarray(paired).view(float) * np.ldexp(1.0, e)[:, None]) * np.ldexp(1.0, -e)[:, None]
    u = v.view(np.uint64).copy()
    u[u == np.uint64(1 << 63)] = 0
    out = u.copy()
    out[1:] ^= u[:-1]
    return out
