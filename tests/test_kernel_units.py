"""No unit compiles a kernel it cannot launch.  hipcc emits a `__global__` function that is not a template into the device code of every
translation unit that sees its definition, launched there or not, so such a kernel belongs in a header that only its launchers include
(kat_amd/csrc/kg_kernels.hpp lists which header holds what).  Text only: the `#include "kg_*.hpp"` closure of every unit of
__graft_entry__.HIP_UNITS, the kernels of those headers that no `template <...>` line precedes, and for each of them the question
whether the unit names it anywhere outside the header that defines it -- in its own text or in another header of its closure, comments
stripped.  No compiler, no GPU."""
import functools
import os
import re

import __graft_entry__ as entry

CSRC = entry.CSRC

_COMMENT = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"(kg_\w+\.hpp)"', re.M)
_KERNEL = re.compile(r'(?:\bstatic\s+)?__global__\s+void\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?(\w+)\s*\(')


@functools.lru_cache(maxsize=None)
def _code(name):
    """The file's text without comments (string and character literals are kept as they are)."""
    with open(os.path.join(CSRC, name)) as f:
        return _COMMENT.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", f.read())


def _closure(unit):
    seen, todo = [], [unit]
    while todo:
        for inc in _INCLUDE.findall(_code(todo.pop())):
            if inc not in seen:
                seen.append(inc)
                todo.append(inc)
    return seen


def _plain_kernels(header):
    """Names of the __global__ definitions of a header that are not templates."""
    text, names = _code(header), []
    for m in _KERNEL.finditer(text):
        before = text[:m.start()].rstrip().rsplit("\n", 1)[-1].lstrip()
        if not before.startswith("template"):
            names.append(m.group(1))
    return names


def _names(text, kernel):
    return re.search(r"\b%s\b" % re.escape(kernel), text) is not None


def test_the_scan_sees_templates_and_plain_kernels():
    # the rule below is only as good as this distinction: one kernel of each kind, where they are known to be
    assert "k_rows_scan" in _plain_kernels("kg_rows_scan.hpp")
    assert "k_count" not in _plain_kernels("kg_kernels.hpp") and _KERNEL.search(_code("kg_kernels.hpp")).group(1) == "k_count"
    assert "kg_kernels.hpp" in _closure("kg_count.hip") and "kg_windows.hpp" in _closure("kg_count.hip")     # (the second: through the first)


def test_no_unit_compiles_a_kernel_it_cannot_launch():
    dead = []
    for unit in entry.HIP_UNITS:
        headers = _closure(unit)
        for h in headers:
            elsewhere = [_code(unit)] + [_code(o) for o in headers if o != h]
            dead += ["%s compiles %s (%s) and never names it" % (unit, k, h) for k in _plain_kernels(h) if not any(_names(t, k) for t in elsewhere)]
    assert not dead, "\n".join(dead)
