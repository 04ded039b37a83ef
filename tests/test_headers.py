"""Every header of figdraw_amd/csrc stands alone: a translation unit that holds nothing but its #include compiles.  The two plain
headers -- the retained scene and the HIP-free vocabulary under it -- also do so for a host compiler that has never heard of HIP."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "figdraw_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))
PLAIN = ("fdh_plain.h", "fdh_retained.h")


def test_the_header_list_is_the_directory():
    assert HEADERS and set(PLAIN) <= set(HEADERS)


@pytest.mark.parametrize("header", HEADERS + [h + " (g++)" for h in PLAIN])
def test_header_compiles_as_the_only_include(header, tmp_path):
    name, plain = header.split(" ")[0], header.endswith("(g++)")
    tu = tmp_path / "only.cpp"
    tu.write_text(f'#include "{name}"\n')
    cmd = (["g++", "-std=c++17", "-fsyntax-only"] if plain else
           [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17", "-fsyntax-only"])
    r = subprocess.run(cmd + ["-I", CSRC, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    text = open(os.path.join(CSRC, name)).read()
    assert "not a header to include on its own" not in text
