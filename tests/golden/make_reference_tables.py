#!/usr/bin/env python3
"""Builds tests/golden/reference_tables.json from DATA tables of the reference tree, read as text, so that the tests that compare the
oracle's and the library's tables with the reference need nothing outside this repository:

  primes, prime_sums   core/src/low_discrepency.rs      PRIMES / PRIME_SUMS (1000 entries each)
  noise_perm           core/src/texture/common.rs       NOISE_PERM (512 entries)
  sobol_sha256         core/src/sobol_matrices.rs       sha256 of the leading part of SOBOL_MATRICES_32 / VD_C_SOBOL_MATRICES /
                                                        VD_C_SOBOL_MATRICES_INV that sobol_subset.npz holds (little-endian u32 / u64 bytes)

    python tests/golden/make_reference_tables.py <reference tree>
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_sobol_fixture as mk  # noqa: E402  (table(): the parser of the Sobol tables' text)


def prime_table(src, name):
    m = re.search(r"pub const %s: \[usize; PRIME_TABLE_SIZE\] = \[(.*?)\];" % name, src, re.S)
    assert m, name
    vals = [int(v) for v in re.findall(r"\d+", m.group(1))]
    assert len(vals) == 1000, (name, len(vals))
    return vals


def noise_perm(src):
    vals = [int(x) for x in re.findall(r"\d+", src[src.index("NOISE_PERM: [usize; 2 * NOISE_PERM_SIZE] = ["):].split("];")[0].split("= [", 1)[1])]
    assert len(vals) == 512, len(vals)
    return vals


def sobol_sha256(src):
    z = np.load(os.path.join(HERE, "sobol_subset.npz"))
    out = {}
    for key, name, dt in (("m32", "SOBOL_MATRICES_32", "<u4"), ("vdc", "VD_C_SOBOL_MATRICES", "<u8"), ("vdc_inv", "VD_C_SOBOL_MATRICES_INV", "<u8")):
        out[key] = hashlib.sha256(np.array(mk.table(src, name)[: len(z[key])], dt).tobytes()).hexdigest()
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    read = lambda p: open(os.path.join(ref, p)).read()
    ld = read("core/src/low_discrepency.rs")
    tables = {"primes": prime_table(ld, "PRIMES"), "prime_sums": prime_table(ld, "PRIME_SUMS"),
              "noise_perm": noise_perm(read("core/src/texture/common.rs")),
              "sobol_sha256": sobol_sha256(read("core/src/sobol_matrices.rs"))}
    out = os.path.join(HERE, "reference_tables.json")
    with open(out, "w") as f:
        json.dump(tables, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
