"""Record tests/golden/noise_table/plain_form.npz: the labels of the pinned cases of
tests/noise_table_cases.py (tests/test_gpu_noise_table.py compares the product with them bitwise).

The fixture is recorded with the plain-form library, so that it checks the table form against the
ten plain Philox rounds:
    python tools/build_variant.py plainfo --units dpi_paths_cha.hip,dpi_paths_ou.hip,dpi_paths_cha_tanh.hip,\
dpi_paths_ou_tanh.hip,dpi_paths_fb_cha.hip,dpi_paths_fb_ou.hip -DDPI_NOISE_TABLE_FO=0
    DPI_HIP_LIB=tools/variants/libdpi_plainfo.so python tools/record_noise_table_golden.py [OUT.npz]
Needs an MI355X.  After an intended change of the label arithmetic, run it again (with the library that
holds the new arithmetic in its plain form) and commit the file."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import noise_table_cases as C  # noqa: E402

out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / C.GOLDEN
arrays = {}
for case in C.PINNED:
    for what, a in C.run(case).items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), (case, what)
        arrays[f"{case}/{what}"] = a
out.parent.mkdir(parents=True, exist_ok=True)
np.savez_compressed(out, **arrays)
print(f"{out}: {len(C.PINNED)} cases, {out.stat().st_size} bytes, library {os.environ.get('DPI_HIP_LIB', 'in-tree')}")
