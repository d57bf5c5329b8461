"""Hashes and staging footprints of the host-pointer call of every case in tests/pointer_cases.py, for comparing two builds
of the library: run once per build, each in a fresh process (AOCLSPARSE_MI355_LIB selects the build), and diff the outputs.

  python tools/staging_evidence.py hashes      ->  <case> <output>=<sha256[:16]> ...
  python tools/staging_evidence.py footprint   ->  <case> <bytes aoclsparse_mi355_release_staging frees after one call>
"""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from pointer_cases import CASES, P, bits, run_case  # noqa: E402


def main(what):
    L = P.lib()
    freed = ctypes.c_size_t()
    for name in sorted(CASES):
        assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
        out, check = run_case(name, "host")
        if what == "hashes":
            print(name, " ".join("%s=%s" % (k, hashlib.sha256(bits(out[k]).tobytes()).hexdigest()[:16]) for k in sorted(out)))
        else:
            assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
            print(name, freed.value)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "hashes")
