"""The hand-kept source lists name exactly the sources on disk (CPU): `_lib.SOURCES`, which `build()` compiles,
and INTEGRATION.md's two build recipes (the shell loop and the `build.rs` example). A source added to or removed
from csrc/ without these lists following either drops out of the library or breaks a maintainer's build."""
import os
import re

from fuzzyheavyhitters_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = re.compile(r"\b\w+\.(?:hip|cpp)\b")


def _on_disk():
    return {f for f in os.listdir(os.path.join(ROOT, "fuzzyheavyhitters_amd", "csrc")) if f.endswith((".hip", ".cpp"))}


def test_lib_sources_match_csrc():
    assert len(set(_lib.SOURCES)) == len(_lib.SOURCES), "a source is listed twice"
    assert set(_lib.SOURCES) == _on_disk()


def test_integration_lists_match_csrc():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    loop = re.search(r"^for f in (.*?); do$", text, re.M | re.S)
    rust = re.search(r"\.args\(\[(\"fhh_[^\]]*)\]", text)
    assert loop and rust, "INTEGRATION.md: the shell loop or the build.rs source list was not found"
    for name, m in (("shell loop", loop), ("build.rs", rust)):
        listed = SOURCE.findall(m.group(1))
        assert len(set(listed)) == len(listed), f"{name}: a source is listed twice"
        assert set(listed) == _on_disk(), name
