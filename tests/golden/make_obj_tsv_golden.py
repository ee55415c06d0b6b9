"""Regenerates tests/golden/obj_tsv_small.tsv and tests/golden/obj_tsv.npz.

The TSV is data: six seeded lines, two each at (O, F) = (1, 8), (2, 8), (3, 8), so that bytes % 3 takes 0, 1 and 2 in every
base64 field, with the special feature values and extreme ids of tests/tsv_cases.py.  The npz holds what the REFERENCE's own
``load_obj_tsv`` (src/utils.py:21-62) returns for that file, item by item under the keys ``"<line>/<field>"`` -- the
reference is imported from its checkout with ``h5py``, absent offline and unrelated to the arithmetic, replaced by an
empty module as make_golden.py does.  Run from the repository root: python tests/golden/make_obj_tsv_golden.py"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/src"

if "h5py" not in sys.modules:
    sys.modules["h5py"] = types.ModuleType("h5py")
sys.path.insert(0, REF)
import utils as ref_utils  # noqa: E402  (the reference's src/utils.py)

import tsv_cases as C  # noqa: E402
from xggm_amd.tools import tsv  # noqa: E402


def main():
    recs = []
    for O, F in C.SMALL:
        recs += [dict(r, img_id="%s_%d" % (r["img_id"], O)) for r in C.records(O, F, 2)]
    path = os.path.join(HERE, "obj_tsv_small.tsv")
    tsv.write_obj_tsv(path, recs)
    items = ref_utils.load_obj_tsv(path)
    assert len(items) == len(recs)
    out = {}
    for i, it in enumerate(items):
        assert list(it.keys()) == ref_utils.FIELDNAMES
        for k, v in it.items():
            out["%d/%s" % (i, k)] = np.asarray(v)
    np.savez(os.path.join(HERE, "obj_tsv.npz"), **out)
    print("wrote %s (%d bytes) and obj_tsv.npz (%d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
