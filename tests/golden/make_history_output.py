"""Writes tests/golden/history_output_parent.nc: the output file restart.write_output makes of tests/test_history.py::output_store().

The committed file was written with the restart.py of the commit BEFORE write_output gained its `more` argument (that commit's
noahmp_amd/restart.py in a copy of the package); tests/test_history.py checks that today's write_output, called without `more`, still
writes it byte for byte.  Re-running this script with the current code must therefore reproduce the committed file.

Usage:  python tests/golden/make_history_output.py [PACKAGE_PARENT_DIR]     (default: this repository)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else ROOT)     # where `noahmp_amd` is taken from
sys.path.insert(1, ROOT)

from noahmp_amd import restart  # noqa: E402
from tests.test_history import output_store  # noqa: E402

if __name__ == "__main__":
    s, extra = output_store()
    out = restart.write_output(os.path.join(HERE, "history_output_parent.nc"), s, "2000-06-28_12:00:00", extra=extra)
    print("wrote", out, os.path.getsize(out), "bytes; restart.py from", restart.__file__)
