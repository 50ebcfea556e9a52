#!/usr/bin/env python3
"""Do two trees compile to the same device code?  (a refactor that claims to leave every kernel as the compiler saw it)
    python tools/asm_identity.py [--pair OLD=NEW ...] <csrc dir A> <csrc dir B> [file.hip ...] [-- <compile flag> ...]
                                                                                                  default file: nmpc_torque.hip
Compiles the named files of both directories to gfx950 device assembly with the compile flags of csrc/build.sh plus
`--cuda-device-only -S` and whatever follows `--` (a diagnostic build: `-- -DNMPC_STAMPS`), drops comments, directives and blank lines, numbers the local labels of each function in order of
appearance and compares the instruction stream function by function.  One line per kernel: its instruction count and `same`
or the number of differing lines; exit status 1 on any difference.  `--pair OLD=NEW` (demangled names without their arguments,
as the report prints them) compares function OLD of A with the differently named NEW of B, a kernel that became an instantiation
of a template for instance; unpaired, one is reported missing and one added.  Each directory has to sit in its tree (the sources
include ../../include); `git worktree add <dir> <commit>` gives one of another commit.  No GPU is needed."""
import difflib, os, re, subprocess, sys, tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-S"]


def functions(csrc, name, tmp, extra=()):
    """{mangled name: [instruction lines]} of one source file"""
    asm = os.path.join(tmp, "out.s")
    subprocess.run(["hipcc", *FLAGS, *extra, os.path.join(csrc, name), "-o", asm], check=True)
    return parsed(asm)


def parsed(asm):
    """{mangled name: [instruction lines]} of a file of device assembly"""
    out, cur, labels = {}, None, {}
    for line in open(asm):
        line = re.sub(r"\s*(;|//).*", "", line).strip()
        m = re.fullmatch(r"\.type\s+(\S+),@function", line)
        if m:
            cur, labels = out.setdefault(m.group(1), []), {}
        elif re.match(r"\.size\s", line):
            cur = None
        elif line and cur is not None and (not line.startswith(".") or line.endswith(":")):
            cur.append(re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line))
    return {k: v[1:] if v and v[0] == k + ":" else v for k, v in out.items()}


def differing(a, b):
    if len(a) == len(b):
        return sum(x != y for x, y in zip(a, b))
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def demangled(k):
    name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
    return re.sub(r"^void ", "", re.sub(r"\(.*", "", name))


def main():
    args, pairs = sys.argv[1:], {}
    while args and args[0] == "--pair":
        old, new = args[1].split("=", 1)
        pairs[new], args = old, args[2:]
    extra = []
    if "--" in args:
        args, extra = args[:args.index("--")], args[args.index("--") + 1:]
    if len(args) < 2:
        sys.exit(__doc__)
    dir_a, dir_b, files = args[0], args[1], args[2:] or ["nmpc_torque.hip"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            a, b = functions(dir_a, f, tmp, extra), functions(dir_b, f, tmp, extra)
            mangled = {demangled(k): k for k in a}
            for new in [k for k in b if pairs.get(demangled(k)) in mangled]:      # NEW of B goes under OLD's mangled name
                b[mangled[pairs[demangled(new)]]] = b.pop(new)
            for k in sorted(set(a) | set(b)):
                name = demangled(k)
                if k not in a or k not in b:
                    verdict = f"only in {dir_a if k in a else dir_b}"
                else:
                    n = differing(a[k], b[k])
                    verdict = "same" if n == 0 else f"{n} lines differ ({len(a[k])} -> {len(b[k])})"
                bad += verdict != "same"
                print(f"{f}: {name}: {sum(not l.endswith(':') for l in a.get(k, b.get(k)))} instructions, {verdict}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
