"""What the device tests of the Fresnel transmittance share (tests/test_transmittance_gpu.py, tests/test_hero_edge_rays_gpu.py): the
lens tables of a hero_cases camera as the host build of csrc/transmittance.hpp takes them, the films of the coated cases, and the
expected T of every column of a batch of records.  A plain helper module."""
import numpy as np

import differentials_ref as dref
import hero_cases as hr
from host_drivers import run_transmittance
from transmittance_ref import films_where_media_differ, housings

F32 = np.float32
_TABLES = {}


def tables(name):
    """(dispersion, surfaces, housing2, film in trace order) of the camera's lens, from a tables-only camera"""
    if name not in _TABLES:
        cam = hr.spec(name).camera(device=-1)
        info, disp = cam.info(), cam.dispersion()
        cam.close()
        _TABLES[name] = disp, dref.surfaces(info), housings(info), films_where_media_differ(disp)
    return _TABLES[name]


def coat(cam, name, coated):
    """the camera, with the films of tables(name) on it where coated"""
    if coated:
        nc, l0 = tables(name)[3]
        cam.set_coatings(nc[::-1], l0[::-1])      # file order
    return cam


def expected(driver, name, coated, starts, here, weights):
    """(n, k) float32: the host build's T from the row's start at the column's wavelength where the record has weight and the
    wavelength is valid, else +0.0"""
    disp, surf, h2, film = tables(name)
    n, k = here.shape
    want = np.zeros((n, k), F32)
    for j in range(k):
        live = (weights[:, j] != 0) & hr.valid(here[:, j])
        rows = np.nonzero(live)[0]
        if len(rows):
            want[rows, j] = run_transmittance(driver, surf, disp, here[rows, j], starts[rows, 0:3], starts[rows, 3:6], film if coated else None, h2)
    return want
