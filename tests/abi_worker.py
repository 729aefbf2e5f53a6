"""The child processes of the plan tests: a fresh interpreter without torch, so that switches the library reads once per
process can be set per case. Standard library only (tests/helpers.py imports torch; this must not).

A worker script is prefixed with BIND, which loads xfmr_rec_amd/_abi.py by file path -- not through the package, which imports
torch -- and binds both signature tables: the script finds `abi` (the Structures), `lib` (typed) and `report(...)`, which
prints its values as one JSON line behind the flag "torch was imported". run_worker returns (that flag, the values); the test
asserts the flag false."""

import json
import pathlib
import subprocess
import sys

ABI_PATH = pathlib.Path(__file__).resolve().parents[1] / "transformer-recommenders_amd" / "xfmr_rec_amd" / "_abi.py"

BIND = f"""
import ctypes as C, importlib.util, json, os, sys
_spec = importlib.util.spec_from_file_location("_abi", {str(ABI_PATH)!r})
abi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(abi)
lib = abi.bind(C.CDLL(sys.argv[1]))
def report(*values):
    print(json.dumps(["torch" in sys.modules, *values]))
"""


def run_worker(script, lib_path, env, stdin=""):
    r = subprocess.run([sys.executable, "-c", BIND + script, str(lib_path)], input=stdin, env=env, capture_output=True,
                       text=True, check=True)
    torch_imported, *values = json.loads(r.stdout)
    return torch_imported, values
