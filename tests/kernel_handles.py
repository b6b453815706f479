"""Helper (no tests): the __global__ instantiations linked into a built library, from its host-side kernel handles (`nm`: one weak object per
template instantiation, one data object per plain kernel, named as the kernel), demangled. Used by the "linked == plannable" tests
(test_kernel_reachability.py, test_fa2_causal_surface.py, test_fa2_bwd_surface.py)."""
import re
import shutil
import subprocess

import pytest

M16X = "fa2::fa2_fwd_m16x_kernel"  # <D, RPW, BC, PD, NDEF, OX, VT, CAUSAL, ORDER, LSE> (csrc/flash_attn_m16x.cuh): every m16x forward of the product


def kernel_handles(so):
    """[(qualified kernel name, [template arguments as text])]"""
    nm, filt = shutil.which("nm"), shutil.which("c++filt")
    if not nm or not filt:
        pytest.skip("binutils nm / c++filt not available")
    out = subprocess.run([nm, so], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "VvWwDd" and "_kernel" in ln and "__device_stub__" not in ln]
    dem = subprocess.run([filt], input="\n".join(n.replace("DF16_", "Dh") for n in names), capture_output=True, text=True, check=True).stdout
    res = []
    for d in dem.splitlines():
        m = re.match(r"(?:void )?((?:\w+::)*\w+_kernel)(?:<(.*?)>)?\(", d)
        if m:
            res.append((m.group(1), [a.strip() for a in (m.group(2) or "").split(",")]))
    return res


# Which "linked == plannable" test answers for a fa2_fwd_m16x_kernel instantiation, by its template arguments CAUSAL (a[7]) and LSE (a[9]):
# plain -> test_kernel_reachability.py, causal -> test_fa2_causal_surface.py, lse (either CAUSAL) -> test_fa2_bwd_surface.py.
# test_kernel_reachability.py holds every linked instantiation to exactly one of them.
M16X_CLAIMS = {
    "plain": lambda a: a[7] == "false" and a[9] == "false",
    "causal": lambda a: a[7] == "true" and a[9] == "false",
    "lse": lambda a: a[9] == "true",
}


def m16x_args(demangled):
    """Template arguments of a demangled fa2_fwd_m16x_kernel name (tools/kernel_resources.py `demangled`), None for any other kernel."""
    m = re.search(re.escape(M16X) + r"<(.*?)>\(", demangled)
    return [a.strip() for a in m.group(1).split(",")] if m else None
