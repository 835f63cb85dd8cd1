"""f64 restatement of the multilayer coatings (zoic_amd/csrc/coating_stack.hpp) for the tests, and the stacks the tests name.  The
reflectance is the GENERAL complex transfer-matrix product in numpy complex128 -- per layer [[cos d, i sin d / eta], [i eta sin d, cos d]]
with d = 2 pi n d cos / lambda, eta = n cos (s) or n / cos (p), r = (eta0 B - C) / (eta0 B + C) for [B, C] = M [1, etas] -- not the
header's real recurrence, its dual p admittance or its scaling.  The rules are the header's: equal media give 1, a layer that
carries no wave ((n1 / n_j)^2 sin^2 i >= 1) gives the bare interface.

The path restatements are the existing ones (transmittance_ref.transmittance, ghost_ref.ghost, traceback_throughput_ref.Throughput):
they price every interface through transmittance_ref.interface_transmittance(n1, n2, ci, ct, nc, lambda0, lam), and `in_force` below
puts a stack-aware version of that one function in its place for the length of a `with` block.  An interface with a stack is marked
in the film-index array those restatements take by the entry STACK_MARK + i.  A helper, not a test."""
import contextlib

import numpy as np

import differentials_spectral_ref as sref
import transmittance_ref as tref

F32 = np.float32
MAX_LAYERS = 8
STACK_MARK = 1000.0

# The stacks the tests name, as (index, thickness nm) pairs, layer 0 adjoining the FRONT-side medium (the C-ABI's order).
Q = [(1.38, 550.0 / (4 * 1.38))]
QHQ = [(1.38, 550.0 / (4 * 1.38)), (2.05, 550.0 / (2 * 2.05)), (1.63, 550.0 / (4 * 1.63))]
_rng = np.random.default_rng(20240808)
R8 = [(float(F32(n)), float(F32(d))) for n, d in zip(_rng.uniform(1.38, 2.4, 8), _rng.uniform(10.0, 300.0, 8))]
THICK = [(4.0, 1000.0)]
NAMED = dict(Q=Q, QHQ=QHQ, R8=R8, THICK=THICK)


def f32_pairs(stack):
    """the stack as the library holds it: every number rounded to f32"""
    return [(float(F32(n)), float(F32(d))) for n, d in stack]


def stack_reflectance(n1, n2, ci, ct, layers, lam):
    """(R_s, R_p, evanescent) of the interface n1 -> n2 through `layers` ((index, nm) IN THE ORDER THE RAY MEETS THEM): arrays broadcast"""
    n1, n2, ci, ct, lam = (np.asarray(a, np.float64) for a in np.broadcast_arrays(n1, n2, ci, ct, lam))
    shape = n1.shape
    sin2 = 1.0 - ci * ci
    Ms = np.broadcast_to(np.eye(2, dtype=np.complex128), shape + (2, 2)).copy()
    Mp = Ms.copy()
    evan = np.zeros(shape, bool)
    with np.errstate(all="ignore"):
        for nj, dj in layers:
            s2 = (n1 / nj) ** 2 * sin2
            evan |= s2 >= 1.0
            cc = np.sqrt(np.where(s2 < 1.0, 1.0 - s2, 1.0))
            delta = 2.0 * np.pi * nj * dj * cc / lam
            c, s = np.cos(delta), np.sin(delta)
            for M, eta in ((Ms, nj * cc), (Mp, nj / cc)):
                layer = np.empty(shape + (2, 2), np.complex128)
                layer[..., 0, 0] = c
                layer[..., 0, 1] = 1j * s / eta
                layer[..., 1, 0] = 1j * eta * s
                layer[..., 1, 1] = c
                M[...] = M @ layer
        out = []
        for M, eta0, etas in ((Ms, n1 * ci, n2 * ct), (Mp, n1 / ci, n2 / ct)):
            B = M[..., 0, 0] + M[..., 0, 1] * etas
            C = M[..., 1, 0] + M[..., 1, 1] * etas
            r = (eta0 * B - C) / (eta0 * B + C)
            # a cosine of 0 is grazing incidence or the critical angle: everything is reflected (the p admittance is infinite there)
            out.append(np.where((ci == 0.0) | (ct == 0.0), 1.0, np.abs(r) ** 2))
    return out[0], out[1], evan


def stack_transmittance(n1, n2, ci, ct, layers, lam):
    """T_i of the interface through `layers` in the order the ray meets them, with the header's rules"""
    n1, n2, ci, ct, lam = (np.asarray(a, np.float64) for a in np.broadcast_arrays(n1, n2, ci, ct, lam))
    Rs, Rp, evan = stack_reflectance(n1, n2, ci, ct, layers, lam)
    with np.errstate(all="ignore"):
        t = np.where(evan, tref.uncoated(n1, n2, ci, ct), 1.0 - (Rs + Rp) / 2.0)
    return np.where(n1 == n2, 1.0, t)


def to_trace_order(stacks_file_order):
    """stacks in FILE order, layer 0 at the front-side medium -> trace order (rear first), layers as a forward ray meets them"""
    return [None if not s else f32_pairs(s)[::-1] for s in list(stacks_file_order)[::-1]]


def table(stacks_trace_order):
    """(layers (count,) int32, index (count, 8), thickness (count, 8) float32) of stacks in trace order: what coating_stacks() returns"""
    count = len(stacks_trace_order)
    layers, index, thick = np.zeros(count, np.int32), np.zeros((count, MAX_LAYERS), F32), np.zeros((count, MAX_LAYERS), F32)
    for i, s in enumerate(stacks_trace_order):
        if s:
            layers[i] = len(s)
            index[i, :len(s)], thick[i, :len(s)] = [p[0] for p in s], [p[1] for p in s]
    return layers, index, thick


def marked_films(stacks_trace_order, films=None):
    """the (index, lambda0) film arrays, trace order, that the path restatements take, with STACK_MARK + i where interface i has a stack"""
    count = len(stacks_trace_order)
    nc = np.zeros(count) if films is None else np.array(films[0], np.float64)
    l0 = np.zeros(count) if films is None else np.array(films[1], np.float64)
    for i, s in enumerate(stacks_trace_order):
        if s:
            nc[i], l0[i] = STACK_MARK + i, 0.0
    return nc, l0


@contextlib.contextmanager
def in_force(stacks_trace_order, disp):
    """within the block transmittance_ref.interface_transmittance prices an interface marked STACK_MARK + i through stack i (trace
    order, layers as a forward ray meets them).  Which way the ray goes is read off its media: forward where n1 is the index BEHIND
    interface i at that wavelength (disp: the camera's dispersion table), backward otherwise."""
    plain = tref.interface_transmittance

    def priced(n1, n2, ci, ct, nc, lambda0, lam):
        if not nc >= STACK_MARK:
            return plain(n1, n2, ci, ct, nc, lambda0, lam)
        i = int(round(float(nc) - STACK_MARK))
        layers = stacks_trace_order[i]
        a1, a2, aci, act, alam = (np.asarray(a, np.float64) for a in np.broadcast_arrays(n1, n2, ci, ct, lam))
        rear = sref.cauchy_index(disp, alam.reshape(-1))[:, i].reshape(alam.shape)
        forward = np.abs(a1 - rear) <= np.abs(a2 - rear)
        return np.where(forward, stack_transmittance(a1, a2, aci, act, layers, alam), stack_transmittance(a1, a2, aci, act, layers[::-1], alam))

    tref.interface_transmittance = priced
    try:
        yield
    finally:
        tref.interface_transmittance = plain


def stacks_where_media_differ(disp, stack, special=None):
    """FILE-order stacks for set_coating_stacks: `stack` (given low-index-first, as on glass under air) on every interface whose media
    differ at the d-line, turned so that its first layer adjoins the medium of lower index; special: {trace index: stack} taken as given"""
    n_rear = np.asarray(disp["ior_d"], np.float64)
    n_front = np.append(n_rear[1:], 1.0)
    out = []
    for i in range(len(n_rear)):
        if special and i in special:
            out.append(list(special[i]))
        elif n_rear[i] == n_front[i]:
            out.append(None)
        else:
            out.append(list(stack) if n_front[i] < n_rear[i] else list(stack)[::-1])
    return out[::-1]
