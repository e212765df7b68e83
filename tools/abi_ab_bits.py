"""usage: SCRI_AMD_LIB_PATH=LIB python tools/abi_ab_bits.py OUT.json -- sha256 of every output of the host / device parity table
(tests/helpers/abi_cases.py: every case in every memory layout it takes); run once per build and compare the files"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scri_amd
from scri_amd import _lib
from tests.helpers import abi_cases

ctx = _lib.Context(0)
print("library", _lib.LIB_PATH, flush=True)
out = {}
for case in abi_cases.CASES:
    for layout in case.layouts:
        for k, a in enumerate(case.run(ctx, layout)):
            out[f"{case.id} {layout} {k}"] = hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
print("hashes", len(out), flush=True)
json.dump(out, open(sys.argv[1], "w"), indent=0, sort_keys=True)
ctx.close()
