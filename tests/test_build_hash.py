"""Each shipped library is tied to the sources it was built from:
the build embeds a hash of its sources, headers and flags, and the loaders refuse a
library whose hash differs from the sources on disk.  CPU only (nothing is launched)."""
from __future__ import annotations

import importlib
import os
import re
import shutil

import pytest

PKG = "adversarial-collaborative-filtering_amd"
bn = importlib.import_module(PKG + ".build_native")
native = importlib.import_module(PKG + "._native")


def _copy_tree(tmp_path, name):
    """The library and exactly the files its hash covers, in the repo layout."""
    spec = bn.LIBS[name]
    for rel in [spec["lib"], *spec["srcs"], *spec["headers"]]:
        dst = tmp_path / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(os.path.join(bn.REPO, rel), dst)
    return str(tmp_path / spec["lib"])


@pytest.mark.parametrize("name", ["apr", "neumf", "torch"])
def test_shipped_libraries_match_their_sources(name):
    path = os.path.join(bn.REPO, bn.LIBS[name]["lib"])
    assert bn.embedded_hash(path) == bn.source_hash(name)
    bn.verify(name)


def test_hash_covers_sources_headers_and_flags(tmp_path):
    _copy_tree(tmp_path, "apr")
    root = str(tmp_path)
    h0 = bn.source_hash("apr", root)
    assert h0 == bn.source_hash("apr")
    hdr = tmp_path / "include" / "acf_apr.h"
    hdr.write_text(hdr.read_text() + "\n/* edited */\n")
    assert bn.source_hash("apr", root) != h0
    flags = list(bn.HIPCC_FLAGS)
    try:
        bn.HIPCC_FLAGS.append("-DX")
        assert bn.source_hash("apr") != h0
    finally:
        bn.HIPCC_FLAGS[:] = flags


@pytest.mark.parametrize("name", ["apr", "neumf", "torch"])
def test_hash_covers_every_included_file(name):
    """Every file a unit of the library pulls in with #include "..." (through other
    headers too) is one of the library's hashed files: an edit to a header that LIBS
    does not list would leave a stale library accepted."""
    spec = bn.LIBS[name]
    dirs = ["include", os.path.join(PKG, "csrc")]  # where the build finds a quoted include
    listed = set(spec["srcs"]) | set(spec["headers"])
    seen, todo = set(), list(spec["srcs"])
    while todo:
        rel = todo.pop()
        if rel in seen:
            continue
        seen.add(rel)
        with open(os.path.join(bn.REPO, rel)) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                found = [os.path.join(d, inc) for d in dirs if os.path.isfile(os.path.join(bn.REPO, d, inc))]
                assert found, f'{rel} includes "{inc}", which is in neither of {dirs}'
                todo.append(found[0])
    assert seen - listed == set(), f"LIBS[{name!r}] does not hash {sorted(seen - listed)}"


def test_load_refuses_library_after_header_edit(tmp_path):
    lib = _copy_tree(tmp_path, "apr")
    root = str(tmp_path)
    bn.verify("apr", lib, root)  # unedited copy: accepted
    hdr = tmp_path / "include" / "acf_apr.h"
    hdr.write_text(hdr.read_text() + "\n/* a declaration changed */\n")
    with pytest.raises(ImportError, match="built from other sources"):
        bn.verify("apr", lib, root)
    saved = native._lib
    native._lib = None  # bypass the process-wide cache for this check
    try:
        with pytest.raises(ImportError, match="built from other sources"):
            native.load(lib, root)
    finally:
        native._lib = saved


def test_load_neumf_refuses_library_after_source_edit(tmp_path):
    lib = _copy_tree(tmp_path, "neumf")
    srcs = bn.LIBS["neumf"]["srcs"]
    assert [os.path.basename(s) for s in srcs] == ["acf_neumf.hip", "acf_keras_mf.hip"]
    saved = native._neumf
    native._neumf = None
    try:
        for rel in srcs:  # an edit to either unit, the other as built
            src = tmp_path / rel
            text = src.read_text()
            src.write_text(text + "\n// edited\n")
            with pytest.raises(ImportError, match="built from other sources"):
                native.load_neumf(lib, str(tmp_path))
            src.write_text(text)
            bn.verify("neumf", lib, str(tmp_path))  # restored: accepted again
    finally:
        native._neumf = saved


def test_unhashed_library_is_refused(tmp_path):
    lib = _copy_tree(tmp_path, "apr")
    data = open(lib, "rb").read().replace(b"ACF_BUILD_HASH=", b"ACF_BUILD_HASX=")
    open(lib, "wb").write(data)
    assert bn.embedded_hash(lib) is None
    with pytest.raises(ImportError):
        bn.verify("apr", lib, str(tmp_path))
