#!/usr/bin/env python3
"""Record what every size function of the C ABI returns (the cases of tests/_scratch_sizes.py) into
tests/golden/scratch_sizes.json, the table tests/test_scratch_layouts_cpu.py holds the library to.  Runs on CPU.

The table is a recording of a build that is KNOWN GOOD, never of the change under test: run this on the commit before a change to
the scratch layouts (GMSPLAT_LIB=/path/to/that/libgmsplat.so selects another checkout's library), and again only when a layout is
changed on purpose.  The library reads GMS_MICRO once per process, so every environment is measured in a child of its own:
"default" with the caller's environment, "GMS_MICRO=0" for gms_binning_bytes without the micro-tile arrays."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "scratch_sizes.json")


def child(which, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_scratch_sizes.py"), which], env=dict(os.environ, **env),
                       capture_output=True, text=True, check=True)
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    table = {"default": child("all", {}), "GMS_MICRO=0": child("binning", {"GMS_MICRO": "0"})}
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]" for k, v in table.items()) + "\n}\n")
    print(f"{OUT}: {sum(len(v) for v in table.values())} records")
