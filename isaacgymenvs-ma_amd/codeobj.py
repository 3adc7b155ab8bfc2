"""Static checks of the gfx950 code objects inside the built library (libmigym.so).

The team kernels must contain no real calls: every phase is force-inlined.  Round 3 saw a
real call into the narrowphase miscompile with this toolchain (wrong object states with IPRA on; an illegal
address and a 93 % parity build with IPRA off), and the inliner has declined a forceinline before (fk(),
DESIGN.md §3 Resources).  ``calls(so)`` lists every ``s_swappc_b64`` (a call) and ``s_setpc_b64 s[30:31]`` (a
return: only a callable function has one; long branches use s_setpc_b64 on other registers) in the device code, per code object, so build.py can fail
the build and tests/test_code_objects.py can assert on the shipped library.

``diff(old_so, new_so)`` compares two builds' device code (section bytes and disassembly, per code object): the
check for a source change that must leave the machine code as it was (tools/codeobj_diff.py).

The fat binary is read without the ROCm bundler: the ELF section ``.hip_fatbin`` holds one clang offload
bundle per translation unit ("__CLANG_OFFLOAD_BUNDLE__", entry count, then (offset, size, triple) per entry),
and the gfx950 entry of each is an AMDGPU ELF that ``llvm-objdump -d`` disassembles.
"""
import os
import re
import struct
import subprocess
import tempfile

def _objdump():
    """llvm-objdump of the ROCm install that builds the library: MIGYM_OBJDUMP, else <root>/lib/llvm/bin/llvm-objdump
    with <root> from ROCM_PATH, or from the hipcc in use (HIPCC, or hipcc on PATH: <root>/bin/hipcc), else /opt/rocm"""
    if os.environ.get("MIGYM_OBJDUMP"):
        return os.environ["MIGYM_OBJDUMP"]
    roots = []
    if os.environ.get("ROCM_PATH"):
        roots.append(os.environ["ROCM_PATH"])
    import shutil
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    roots.append("/opt/rocm")
    for r in roots:
        cand = os.path.join(r, "lib", "llvm", "bin", "llvm-objdump")
        if os.path.exists(cand):
            return cand
    raise FileNotFoundError("codeobj: no llvm-objdump under " + ", ".join(f"{r}/lib/llvm/bin" for r in roots) +
                            "; set MIGYM_OBJDUMP to its path (or ROCM_PATH to the ROCm root)")


def have_objdump():
    try:
        return os.path.exists(_objdump())
    except FileNotFoundError:
        return False


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _section(path, name, d=None):
    """section `name` of the ELF64 file at `path` (or of the image `d`, `path` then only names it in errors)"""
    if d is None:
        d = open(path, "rb").read()
    if d[:4] != b"\x7fELF" or d[4] != 2:
        raise ValueError(f"{path}: not an ELF64 file")
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    strtab = hdrs[shstrndx]
    for h in hdrs:
        nm = d[strtab[4] + h[0]:d.index(b"\0", strtab[4] + h[0])].decode()
        if nm == name:
            return d[h[4]:h[4] + h[5]]
    raise ValueError(f"{path}: no {name} section")


def device_code_objects(so, arch="gfx950"):
    """the AMDGPU code objects (bytes) of every offload bundle in the library's .hip_fatbin"""
    fb = _section(so, ".hip_fatbin")
    out = []
    i = fb.find(MAGIC)
    while i >= 0:
        n, = struct.unpack_from("<Q", fb, i + len(MAGIC))
        p = i + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fb, p)
            triple = fb[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.startswith("hip") and triple.endswith(arch):
                out.append(fb[i + off:i + off + size])
        i = fb.find(MAGIC, i + 1)
    return out


def _disassemble(co, arch):
    """``llvm-objdump -d`` of one code object (bytes), without the header lines that carry the file's name"""
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "co.o")
        with open(f, "wb") as fh:
            fh.write(co)
        txt = subprocess.run([_objdump(), "-d", f"--mcpu={arch}", f], capture_output=True, text=True, check=True).stdout
    return [line for line in txt.splitlines() if "file format" not in line]


def _functions(lines):
    """{function: its lines} of a disassembly"""
    fns, fn = {}, "?"
    for line in lines:
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            fn = m.group(1)
        fns.setdefault(fn, []).append(line)
    return fns


def calls(so, arch="gfx950"):
    """[(code object index, function, instruction)] for every call / return in the device code"""
    found = []
    for k, co in enumerate(device_code_objects(so, arch)):
        for fn, lines in _functions(_disassemble(co, arch)).items():
            for line in lines:
                if "s_swappc_b64" in line or re.search(r"s_setpc_b64\s+s\[30:31\]", line):
                    # a call, or a return through the return address (s[30:31]): a callable function.  Long
                    # branches (s_getpc_b64 + add + s_setpc_b64 on other registers) are kernels' own jumps
                    found.append((k, fn, line.split()[0]))
    return found


def check_no_calls(so, arch="gfx950"):
    bad = calls(so, arch)
    if bad:
        fns = sorted({f for _, f, _ in bad})
        raise RuntimeError(f"{so}: the device code has real calls / returns (the team kernels must be fully "
                           f"inlined, DESIGN.md §3b): {fns[:8]}")
    return True


def diff(old_so, new_so, arch="gfx950"):
    """Compare the device code of two built libraries, code object by code object in .hip_fatbin order: the
    ``.text`` and ``.rodata`` bytes (code and kernel descriptors) and the disassembly.  Returns (code objects
    compared, [(code object index, sections whose bytes differ, functions whose disassembly differs)]); an empty
    list is the same machine code, which is what a source change meant to move none has to show.  A function counts
    as different when its instructions or their encodings do, not when it merely sits at another address behind
    one that grew.  A code object that only one library has is listed with every function it holds."""
    def body(lines):  # a function's instructions and encodings: without its header line and the address column,
        # and without the blank and "..." lines objdump prints for the padding up to whatever function follows
        return [re.sub(r"// [0-9A-F]+:", "//", line) for line in lines[1:] if line.strip() not in ("", "...")]

    def sect(co, name):
        try:
            return _section("code object", name, co)
        except ValueError:
            return b""

    old, new = device_code_objects(old_so, arch), device_code_objects(new_so, arch)
    out = []
    for k in range(max(len(old), len(new))):
        if k >= len(old) or k >= len(new):
            only = old[k] if k < len(old) else new[k]
            out.append((k, ["missing"], sorted(_functions(_disassemble(only, arch)))))
            continue
        secs = [n for n in (".text", ".rodata") if sect(old[k], n) != sect(new[k], n)]
        a, b = _disassemble(old[k], arch), _disassemble(new[k], arch)
        if secs or a != b:
            fa, fb = _functions(a), _functions(b)
            out.append((k, secs, sorted(f for f in set(fa) | set(fb)
                                        if f not in fa or f not in fb or body(fa[f]) != body(fb[f]))))
    return max(len(old), len(new)), out
