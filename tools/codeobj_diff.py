#!/usr/bin/env python3
"""Do two builds of the library hold the same gfx950 machine code?  (codeobj.diff: .text / .rodata bytes and the
disassembly of every code object.)  Exit status 1 if any code object differs.

usage: python tools/codeobj_diff.py OLD.so NEW.so
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "isaacgymenvs-ma_amd"))
import codeobj  # noqa: E402

if len(sys.argv) != 3:
    sys.exit(__doc__)
n, changed = codeobj.diff(sys.argv[1], sys.argv[2])
for k, secs, fns in changed:
    print(f"code object {k}: {', '.join(secs) or 'disassembly'} differ; {len(fns)} functions differ")
    for f in fns:
        print("   ", f)
print(f"{n - len(changed)} of {n} code objects identical")
sys.exit(1 if changed else 0)
