"""fr_forward_ext (include/fovraster.h): the symbols added beside fr_forward_args without an ABI bump -- exported, laid out
in ctypes as in C, and optional: a library of the same ABI version without them loads, and the callers compute the mask."""
import ctypes as C
import subprocess

import torch

from tests.helpers import ROOT
from fov3dgs_amd import _native, rasterizer


def test_the_library_exports_the_ext_entry_points():
    lib = _native.load()
    for name in _native.OPTIONAL_EXPORTS:
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert _native.has_forward_ext(lib) and _native.has_forward_ext()
    assert lib.fr_abi_version() == _native.ABI_VERSION == 12  # (added symbols, same fr_forward_args)
    # the old entry points are the new ones with ext == NULL: both reject the same bad arguments before anything runs
    a = _native.ForwardArgs()
    a.variant = 8
    handle = C.c_void_p()
    assert lib.fr_forward_ext_call(C.byref(a), None) == -1 and b"variant" in lib.fr_last_error()
    assert lib.fr_forward_begin_ext(C.byref(a), None, C.byref(handle)) == -1 and not handle.value
    # ... and a struct from a caller compiled against a shorter fr_forward_ext is refused, not read past its end
    a.variant, a.P, a.W, a.H, a.out_color = 0, 0, 16, 16, 1
    ext = _native.ForwardExt(4, None)
    assert lib.fr_forward_ext_call(C.byref(a), C.byref(ext)) == -1 and b"fr_forward_ext.size" in lib.fr_last_error()


def test_forward_ext_matches_the_c_layout(tmp_path):
    fields = [f[0] for f in _native.ForwardExt._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fovraster.h"', 'int main(){',
            'printf("%zu\\n", sizeof(fr_forward_ext));']
    body += [f'printf("%zu\\n", offsetof(fr_forward_ext, {f}));' for f in fields]
    body += ['return 0;}']
    src, exe = tmp_path / "layout_ext.c", tmp_path / "layout_ext"
    src.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == C.sizeof(_native.ForwardExt)
    assert fields == ["size", "visibility"]
    for f, off in zip(fields, nums[1:]):
        assert getattr(_native.ForwardExt, f).offset == off, f


class _OldLibrary:
    """The loaded library as one built before the ext entry points: every attribute but those two."""

    def __init__(self, lib, calls=None):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        if name in _native.OPTIONAL_EXPORTS:
            raise AttributeError(name)
        if name == "fr_forward_begin" and self._calls is not None:
            # (no GPU here: the call is refused once it is known which entry point was taken)
            return lambda a, handle: self._calls.append(name) or -1
        return getattr(self._lib, name)


def test_a_library_without_the_symbols_loads_and_python_falls_back(monkeypatch):
    calls = []
    real = _native.load()
    old = _OldLibrary(real)
    assert not _native.has_forward_ext(old)
    # load(): the two names are the only ones a library may lack
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native.C, "CDLL", lambda path: old)
    try:
        assert _native.load() is old
    finally:
        monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.undo()
    assert _native.load() is real
    old = _OldLibrary(real, calls)
    # _begin_call: fr_forward_begin, no mask attached to radii -> visibility_of computes it, the result object carries None
    radii = torch.tensor([0, 3, 0, 7], dtype=torch.int32)
    rc = rasterizer._begin_call(old, _native.ForwardArgs(), 4, radii.device, radii, C.c_void_p())
    assert rc == -1 and calls == ["fr_forward_begin"]
    assert getattr(radii, "_fovraster_visibility", None) is None
    vis = rasterizer.visibility_of(radii)
    assert vis.dtype == torch.bool and vis.tolist() == [False, True, False, True]
    out = rasterizer._raster_output((torch.zeros(3, 2, 2), radii))
    assert isinstance(out, tuple) and len(out) == 2 and out[1] is radii and out.visibility_filter is None
    # with a mask beside the radii both hand out the mask itself
    radii._fovraster_visibility = mask = torch.tensor([False, True, False, True])
    assert rasterizer.visibility_of(radii) is mask and rasterizer._raster_output((out[0], radii)).visibility_filter is mask
