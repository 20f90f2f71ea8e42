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


def test_only_the_generic_chain_units_reach_the_chain_and_the_libm_tables():
    """The include closure of every source: the generic kernel's chain
    (h2s_chain.h) and the libm tables under it (h2s_libm.h) are reached by the
    three units that call them and by no tile, host or preview unit; the old
    catch-all header is gone."""
    import glob
    import os
    import re

    direct, text = {}, {}
    for path in glob.glob(os.path.join(_build.CSRC, '*')):
        with open(path, encoding='utf-8') as fh:
            text[os.path.basename(path)] = fh.read()
    for name, body in text.items():
        direct[name] = set(re.findall(r'^\s*#\s*include\s+"(h2s_[^"]+\.h)"', body, re.M))

    def closure(name):
        seen, todo = set(), [name]
        while todo:
            for h in direct[todo.pop()]:
                if h not in seen:
                    seen.add(h)
                    todo.append(h)
        return seen

    assert sorted(_build.SOURCES) == sorted(n for n in text if not n.endswith('.h'))
    for header in ('h2s_chain.h', 'h2s_libm.h'):
        reach = sorted(s for s in _build.SOURCES if header in closure(s))
        assert reach == ['h2s_kernels.hip', 'h2s_peak.hip', 'h2s_testhooks.hip'], header
    assert [n for n, body in sorted(text.items()) if 'h2s_device.h' in body] == []
    assert [n for n in sorted(direct) if 'h2s_libm.h' in direct[n]] == ['h2s_chain.h']
