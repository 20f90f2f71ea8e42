"""The in-tree build (hdr2sdr/_build.py): the gpurun snapshot carries
libh2s.so and its flag stamp but not the objects (build/ is gpurun-ignored),
so a current library must not be recompiled on the GPU box; a flag change
still rebuilds."""
import pytest

from hdr2sdr import _build


class _Compiled(Exception):
    pass


def _no_compiler(*a, **k):
    raise _Compiled(a[0] if a else k)


def test_a_current_library_without_its_objects_is_not_rebuilt(tmp_path, monkeypatch):
    monkeypatch.setattr(_build, 'OBJ_DIR', str(tmp_path / 'obj'))
    monkeypatch.setattr(_build.subprocess, 'run', _no_compiler)
    assert _build.build_lib() == _build.LIB


def test_a_flag_change_rebuilds(tmp_path, monkeypatch):
    monkeypatch.setattr(_build, 'OBJ_DIR', str(tmp_path / 'obj'))
    monkeypatch.setattr(_build.subprocess, 'run', _no_compiler)
    monkeypatch.setattr(_build, '_hipcc', lambda: 'hipcc')
    monkeypatch.setattr(_build, 'CFLAGS', _build.CFLAGS + ['-DH2S_FLAG_CHANGED'])
    with pytest.raises(_Compiled):
        _build.build_lib()


def test_every_included_project_header_is_a_build_dependency():
    """A header that csrc/ includes and HEADERS lacks would leave objects
    current after an edit to it."""
    import glob
    import os
    import re

    included = set()
    for path in glob.glob(os.path.join(_build.CSRC, '*')):
        with open(path, encoding='utf-8') as fh:
            included.update(re.findall(r'^\s*#\s*include\s+"(h2s_[^"]+\.h)"', fh.read(), re.M))
    assert included, 'no project header found: the pattern no longer matches the sources'
    assert sorted(included - set(_build.HEADERS)) == []
    assert all(os.path.exists(os.path.join(_build.CSRC, h)) for h in _build.HEADERS)
