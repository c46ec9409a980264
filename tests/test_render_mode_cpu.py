"""Render mode of the outlier test without a device: the ABI's default and version, the ctypes mirror of the new config field,
and the optional configuration key outlier_rejection.render_mode (roft_amd/config.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from roft_amd import _lib as L
from roft_amd import config as K
from roft_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    text = open(os.path.join(ROOT, "include", "roft_engine.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_default_render_mode_is_the_contract():
    cfg = L.Config()
    assert L.lib().roft_default_config(C.byref(cfg), 640, 480, L.FLOW_F32C2) == 0
    assert cfg.render_mode == 0 == L.RENDER_CONTRACT == _header_define("ROFT_RENDER_CONTRACT")
    assert L.RENDER_GL == _header_define("ROFT_RENDER_GL") == 1
    assert E.default_config(640, 480).render_mode == 0
    assert E.default_config(640, 480, render_mode=L.RENDER_GL).render_mode == 1


def test_abi_version_matches_the_header():
    lib = L.lib()
    assert lib.roft_abi_version() == _header_define("ROFT_ABI_VERSION") == L.ABI_VERSION


def test_render_mode_field_sits_where_the_header_puts_it():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "roft_engine.h"\n'
           'int main(){printf("%zu %zu\\n", offsetof(roft_config, render_mode), sizeof(roft_config));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "o.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "o.c"), "-o", os.path.join(d, "o")])
        off, size = (int(x) for x in subprocess.check_output([os.path.join(d, "o")]).split())
    assert off == L.Config.render_mode.offset and size == C.sizeof(L.Config)


def _parsed(extra=""):
    text = K.default_text(640, 480, 614.7, 614.7, 320.0, 240.0)
    if extra:
        text = text.replace("gain = 0.01;", "gain = 0.01; " + extra)
    return K.parse_cfg(text)


def test_config_key_absent_contract_gl_and_bad():
    cfg = _parsed()
    with pytest.raises(KeyError):
        K.lookup(cfg, "outlier_rejection.render_mode")      # (the defaults file stays one the reference reads)
    assert K.to_engine(cfg, L.FLOW_F32C2)[0].render_mode == L.RENDER_CONTRACT
    assert K.to_engine(_parsed('render_mode = "contract";'), L.FLOW_F32C2)[0].render_mode == L.RENDER_CONTRACT
    assert K.to_engine(_parsed('render_mode = "gl";'), L.FLOW_F32C2)[0].render_mode == L.RENDER_GL
    for bad in ('"GL"', '"opengl"', "1", "true"):
        with pytest.raises(ValueError):
            K.to_engine(_parsed("render_mode = %s;" % bad), L.FLOW_F32C2)
    assert "outlier_rejection.render_mode" not in K.FILTER_KEYS


def test_config_key_through_the_command_line_overrides():
    cfg = _parsed()
    assert K.apply_overrides(cfg, ["--outlier_rejection::render_mode", "gl", "--other", "x"]) == ["--other", "x"]
    assert K.to_engine(cfg, L.FLOW_F32C2)[0].render_mode == L.RENDER_GL
    cfg = _parsed('render_mode = "gl";')
    K.apply_overrides(cfg, ["--outlier_rejection::render_mode", "contract"])
    assert K.to_engine(cfg, L.FLOW_F32C2)[0].render_mode == L.RENDER_CONTRACT
    cfg = _parsed()
    K.apply_overrides(cfg, ["--outlier_rejection::render_mode", "vulkan"])
    with pytest.raises(ValueError):
        K.to_engine(cfg, L.FLOW_F32C2)


def test_config_text_writes_the_key_only_when_it_is_not_the_default():
    assert "render_mode" not in K.default_text(640, 480, 614.7, 614.7, 320.0, 240.0)
    text = K.default_text(640, 480, 614.7, 614.7, 320.0, 240.0, render_mode=L.RENDER_GL)
    assert K.lookup(K.parse_cfg(text), "outlier_rejection.render_mode") == "gl"
    assert K.to_engine(K.parse_cfg(text), L.FLOW_F32C2)[0].render_mode == L.RENDER_GL
