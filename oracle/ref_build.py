"""Recipe for the reference binaries under oracle/_ref/ (git-ignored; built only where a checkout of the reference is at hand).

The reference's two executables -- src/roft/src/main.cpp (ROFT-tracker) and tools/nvof/dumper/src/main.cpp (ROFT-of-dumper) --
compiled UNMODIFIED where they lie, against this repository's class facade (include/ROFT, include/compat) and linked with
libroft_hip.so.  They are the reference's command-line front ends over THIS engine: a compatibility test of the drop-in API
(tests/test_facade.py), not an oracle -- nothing is compared against them as one.  Nothing of the reference is copied here.

The checkout is looked for in $ROFT_REFERENCE_DIR, else in a directory `reference` next to this repository.  Where there is
none, build() builds nothing and leaves whatever oracle/_ref/ already holds.
"""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
OUT = os.path.join(_HERE, "_ref")
TRACKER = os.path.join(OUT, "ROFT-tracker")
DUMPER = os.path.join(OUT, "ROFT-of-dumper")

# (executable, source relative to the reference checkout)
SOURCES = [(TRACKER, os.path.join("src", "roft", "src", "main.cpp")),
           (DUMPER, os.path.join("tools", "nvof", "dumper", "src", "main.cpp"))]


def reference_dir():
    for d in (os.environ.get("ROFT_REFERENCE_DIR", ""), os.path.join(os.path.dirname(ROOT), "reference")):
        if d and os.path.isfile(os.path.join(d, SOURCES[0][1])):
            return d
    return None


def build():
    """Compile what the reference checkout provides into oracle/_ref/; returns the executables built (none without a checkout)."""
    ref = reference_dir()
    if ref is None:
        return []
    os.makedirs(OUT, exist_ok=True)
    csrc = os.path.join(ROOT, "roft_amd", "csrc")
    built = []
    for exe, rel in SOURCES:
        src = os.path.join(ref, rel)
        if not os.path.isfile(src):
            continue
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include", "compat"), "-I", os.path.join(ROOT, "include"), src,
                               "-o", exe, "-L", csrc, "-lroft_hip", "-L/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath,$ORIGIN/../../roft_amd/csrc", "-Wl,-rpath,/opt/rocm/lib"])
        built.append(exe)
    return built
