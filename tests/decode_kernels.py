"""The decode attention kernels of a built library, under the labels the describe texts give them (csrc/flash_attn_decode*.{cuh,hip}):
  ("fa2_decode", D)                    fa2d::fa2_decode_kernel<D, 1, fa2d::DenseKV>
  ("fa2_decode_paged", D, G)           fa2d::fa2_decode_kernel<D, G, fa2d::PagedKV>
  ("fa2_decode_paged_multi", D, MT)    fa2pm::fa2_decode_paged_multi_kernel<D, MT>
  ("fa2_decode_combine", D)            fa2d::fa2_decode_combine_kernel<D>
Shared by the "linked == plannable" tests of the three test_fa2_decode*_surface.py files."""
import re
import shutil
import subprocess

import pytest

NAMESPACES = ("fa2d::", "fa2p::", "fa2pm::")
LABEL = re.compile(r"(fa2_decode(?:_paged(?:_multi)?|_combine)?)<D=(\d+)(?:,(?:G|MT)=(\d+))?>")


def label(demangled):
    """The label of a demangled kernel symbol of the decode namespaces; None for any other symbol. A kernel of these namespaces that has no label
    is an error: the library must hold nothing else from them."""
    mm = re.match(r"(?:void )?((?:\w+::)*\w+_kernel)(?:<(.*?)>)?\(", demangled)
    if not mm or not mm.group(1).startswith(NAMESPACES):
        return None
    name, args = mm.group(1), [a.strip() for a in (mm.group(2) or "").split(",")]
    if name == "fa2d::fa2_decode_combine_kernel" and len(args) == 1:
        return ("fa2_decode_combine", int(args[0]))
    if name == "fa2pm::fa2_decode_paged_multi_kernel" and len(args) == 2:
        return ("fa2_decode_paged_multi", int(args[0]), int(args[1]))
    if name == "fa2d::fa2_decode_kernel" and len(args) == 3 and args[2] == "fa2d::PagedKV":
        return ("fa2_decode_paged", int(args[0]), int(args[1]))
    if name == "fa2d::fa2_decode_kernel" and args[1:] == ["1", "fa2d::DenseKV"]:
        return ("fa2_decode", int(args[0]))
    raise AssertionError("a decode kernel no describe text can name: " + demangled)


def linked(so):
    """The set of labels of the decode kernels linked into the shared object."""
    nm, filt = shutil.which("nm"), shutil.which("c++filt")
    if not nm or not filt:
        pytest.skip("binutils nm / c++filt not available")
    out = subprocess.run([nm, so], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "VvWwDd" and "_kernel" in ln and "__device_stub__" not in ln]
    dem = subprocess.run([filt], input="\n".join(n.replace("DF16_", "Dh") for n in names), capture_output=True, text=True, check=True).stdout
    return {k for k in map(label, dem.splitlines()) if k}


def named(text):
    """The set of labels a describe text names."""
    return {(m[0],) + tuple(int(x) for x in m[1:] if x) for m in LABEL.findall(text)}
