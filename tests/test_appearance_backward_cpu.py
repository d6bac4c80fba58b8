"""fr_backward_appearance (the backward pass of the mask-learning step: gradients of the opacity and the DC colour only) as the C ABI
sees it: a symbol added beside fr_backward over the UNCHANGED fr_backward_args -- same ABI version, same struct size."""
import ctypes as C
import os
import subprocess

from tests.helpers import ROOT
from fov3dgs_amd import _native

# sizeof(fr_backward_args) of ABI version 12 (LP64): pinned so that the new entry point cannot have grown the struct it shares
BACKWARD_ARGS_BYTES = 320


def test_library_exports_the_appearance_backward():
    lib = _native.load()
    assert "fr_backward_appearance" in _native.EXPORTS and "fr_backward_appearance" not in _native.OPTIONAL_EXPORTS
    assert hasattr(lib, "fr_backward_appearance")
    assert lib.fr_backward_appearance.restype is C.c_int
    assert lib.fr_abi_version() == 12 == _native.ABI_VERSION


def test_header_declares_it_over_the_unchanged_struct(tmp_path):
    """The compile-a-snippet method of test_host_cpu.py: the header declares the symbol with fr_backward's signature, the version
    macro is still 12 and the struct has the size it had before the symbol was added."""
    src = tmp_path / "decl.c"
    src.write_text("\n".join([
        '#include <stdio.h>', f'#include "{os.path.join(ROOT, "include", "fovraster.h")}"',
        'int (*fn)(const fr_backward_args *) = fr_backward_appearance; /* the declared signature, checked by -Werror */',
        'int (*full)(const fr_backward_args *) = fr_backward;',
        'int main(void){ printf("%d %zu\\n", FR_ABI_VERSION, sizeof(fr_backward_args)); return 0; }']))
    obj = tmp_path / "decl.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-o", str(obj), str(src)])
    # (sizes from a program that does not reference the library: it runs anywhere)
    size = tmp_path / "size.c"
    size.write_text("\n".join(['#include <stdio.h>', f'#include "{os.path.join(ROOT, "include", "fovraster.h")}"',
                               'int main(void){ printf("%d %zu\\n", FR_ABI_VERSION, sizeof(fr_backward_args)); return 0; }']))
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-o", str(exe), str(size)])
    version, nbytes = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert version == 12
    assert nbytes == BACKWARD_ARGS_BYTES == C.sizeof(_native.BackwardArgs)


def test_forbidden_pointers_and_null_args_are_reported():
    """Validation happens before anything touches the GPU: a pointer for a gradient this pass does not compute is refused by name."""
    lib = _native.load()
    assert lib.fr_backward_appearance(None) == -1
    a = _native.BackwardArgs()
    a.variant = 3
    assert lib.fr_backward_appearance(C.byref(a)) == -1 and b"backward exists only" in lib.fr_last_error()
    for field in ("dL_dmean2D", "dL_dconic", "dL_dmean3D", "dL_dcov3D", "dL_dscale", "dL_drot", "dL_dsh_rest"):
        a = _native.BackwardArgs()
        a.variant, a.P = 1, 5
        setattr(a, field, 4096)
        assert lib.fr_backward_appearance(C.byref(a)) == -1, field
        assert field.encode() in lib.fr_last_error(), (field, lib.fr_last_error())
    a = _native.BackwardArgs()
    a.variant, a.P = 1, 0
    assert lib.fr_backward_appearance(C.byref(a)) == 0  # P == 0: nothing to do, as fr_backward
