"""What a public header declares and what a built library exports: helpers of
the companion libraries' CPU tests (plain functions, no fixtures)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    """The function names include/<header> declares."""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#"))
    src = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", " ", src, flags=re.S)
    return set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", src)) - {"sizeof"}


def exported(path):
    """{name: version node} of the defined dynamic function symbols."""
    out = subprocess.check_output(["objdump", "-T", path], text=True)
    seen = {}
    for line in out.splitlines():
        parts = line.split()
        if len(parts) >= 6 and parts[1] == "g" and "DF" in parts and ".text" in parts:
            seen[parts[-1]] = parts[-2]
    return seen


def c_functions(path):
    """exported(path) without the loader's hooks and the kernels' host stubs."""
    return {n: v for n, v in exported(path).items()
            if n not in ("_init", "_fini") and not (n.startswith("_ZN") and "_kernel" in n)}
