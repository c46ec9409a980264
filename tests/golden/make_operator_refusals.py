"""Writes tests/golden/operator_refusals.json: return code and error string of every row of tests/test_operator_refusals_cpu.py, as
the loaded library answers them (ROFT_LIB_SO names another build than the tree's).  The file has two records, "no_device" and
"device"; a run fills the one of the machine it runs on and keeps the other, so the fixture is complete after one run on each kind
of machine.  The stored file is the record of the library BEFORE the operators moved onto one context: do not regenerate it from a
library whose refusals are under test.

    python tests/golden/make_operator_refusals.py [output file, default: the fixture itself]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_operator_refusals_cpu as T  # noqa: E402
from roft_amd import _lib as L  # noqa: E402

data = {}
if os.path.exists(T.GOLDEN):
    with open(T.GOLDEN) as f:
        data = json.load(f)
key = "device" if L.lib().roft_device_count() > 0 else "no_device"
data[key] = T.record(L.lib())
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
with open(out, "w") as f:
    json.dump(data, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote the %r record: %d rows of %d entry points -> %s" % (key, sum(len(v) for v in data[key].values()), len(data[key]), out))
