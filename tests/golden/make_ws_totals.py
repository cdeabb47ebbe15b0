"""tests/golden/make_ws_totals.py -- regenerates tests/golden/ws_totals.json: crf_workspace_bytes and the two alignment workspaces over the
matrix of tests/test_ws_sections.py, from the library of the commit the packed layout is to be compared with.

Build that commit's library in a scratch checkout (python -m cat_amd.build there), then, from this repo's root:
    CRF_LIB=<scratch>/cat_amd/lib/libctc_crf_hip.so python tests/golden/make_ws_totals.py
(CRF_LIB makes the binding load that library; only exports that commit has are called.)"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    import ctc_crf
    from tests.test_ws_sections import GOLDEN, totals
    print("library:", ctc_crf._C.LIB_PATH)
    with tempfile.TemporaryDirectory() as tmp:
        out = totals(ctc_crf._C, tmp)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "totals ->", GOLDEN)
