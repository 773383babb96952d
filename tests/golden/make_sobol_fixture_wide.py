#!/usr/bin/env python3
"""Builds tests/golden/sobol_subset_64.npz: the first 64 dimensions (52 u32 each) and the first 9 VdC matrices of the reference's Sobol generator-matrix DATA tables, read as
make_sobol_fixture.py reads them.  A path of depth 5 draws 5 + 8 * 6 = 53 dimensions, five more than sobol_subset.npz holds; the tests that render Sobol films at that depth
(tests/test_quadric_alpha_gpu.py) load this file.  Run where the reference tree exists:

    python tests/golden/make_sobol_fixture_wide.py
"""
import os

import numpy as np

import make_sobol_fixture as M

N_DIMS, N_M = 64, 9


def main():
    src = open(M.REF).read()
    m32 = np.array(M.table(src, "SOBOL_MATRICES_32"), dtype=np.uint32)
    vdc = np.array(M.table(src, "VD_C_SOBOL_MATRICES"), dtype=np.uint64)
    vdci = np.array(M.table(src, "VD_C_SOBOL_MATRICES_INV"), dtype=np.uint64)
    assert m32.size == 1024 * 52 and vdc.size == 25 * 52 and vdci.size == 26 * 52, (m32.size, vdc.size, vdci.size)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sobol_subset_64.npz")
    np.savez_compressed(out, m32=m32[: N_DIMS * 52], vdc=vdc[: N_M * 52], vdc_inv=vdci[: N_M * 52])
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
