"""Per-kernel comparison of two device-assembly dumps of csrc/conv1d.hip: do the kernels of PARENT keep their instruction
streams in NEW?  Made for the LENS template parameter: a kernel of NEW whose name is a parent kernel's with a
trailing `false` (or none) is that kernel's DENSE form and must be identical line for line; one with a trailing `true` is the new
ragged form, listed beside the kernel it was made from with registers / scratch / LDS before -> after.

  hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffast-math -fno-finite-math-only --cuda-device-only -S conv1d.hip -o X.s   (both trees)
  python tools/conv_isa_compare.py PARENT.s NEW.s

Compared: every line of a kernel's body, comments stripped, local labels renumbered away (.LBB<function index>_<n> carries the
function's index in the file), the kernel's own symbol replaced by SELF.  Exit status 1 if a dense form differs or is missing."""
import re
import shutil
import subprocess
import sys


def load(path):
    txt = open(path).read()
    funcs = {}
    for m in re.finditer(r'^(_Z\w+):\s*;\s*@\1\n(.*?)^\.Lfunc_end\d+:', txt, flags=re.S | re.M):
        lines = [re.sub(r'\.(LBB|Ltmp|LJTI)\d+_', r'.\1_', ln.split(';')[0].rstrip()) for ln in m.group(2).split('\n')]
        funcs[m.group(1)] = [ln for ln in lines if ln.strip()]
    meta = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', txt, flags=re.S):
        g = lambda k: int(re.search(r'\.amdhsa_' + k + r' (\d+)', m.group(2)).group(1))  # noqa: E731
        meta[m.group(1)] = dict(lds=g('group_segment_fixed_size'), scratch=g('private_segment_fixed_size'), vgpr=g('next_free_vgpr'),
                                sgpr=g('next_free_sgpr'))
    return funcs, meta


def demangled(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    norm = lambda d: re.sub(r'std::conditional<(true|false), Conv(C?)ParamsL, ConvC?Params>::type', r'Conv\2Params',  # noqa: E731
                            re.sub(r'^void ', '', re.sub(r'\(anonymous namespace\)::', '', d)))
    return {n: norm(d) for n, d in zip(names, out)}


def main(parent, new):
    pf, pm = load(parent)
    nf, nm = load(new)
    pkey = {d: k for k, d in demangled(list(pf)).items()}
    rows, bad, kept = [], 0, set()
    for k, d in demangled(list(nf)).items():
        kind, cand, dd = "same name", pkey.get(d), d
        if cand is None:
            dd = re.sub(r'<false>\(', '(', re.sub(r', false>\(', '>(', d))
            kind, cand = "DENSE", pkey.get(dd)
        if cand is None:
            dd = re.sub(r'<true>\(', '(', re.sub(r', true>\(', '>(', d))
            kind, cand = "LENS", pkey.get(dd)
        if cand is None:
            rows.append(("NEW", d, None))
            continue
        same = [ln.replace(cand, 'SELF') for ln in pf[cand]] == [ln.replace(k, 'SELF') for ln in nf[k]]
        bad += kind != "LENS" and not same
        rows.append((kind, dd, same, len(pf[cand]), len(nf[k]), pm[cand], nm[k]))
        if kind != "LENS":
            kept.add(dd)
    for r in sorted(rows, key=lambda r: (r[0], r[1])):
        name = re.sub(r'\((ConvC?Params|[^()]*\*[^()]*)\)$', '', r[1])
        if r[2] is None:
            print(f"{r[0]:9s} (no kernel of the parent) {name}")
            continue
        p, n = r[5], r[6]
        print(f"{r[0]:9s} {'identical' if r[2] else 'differs  '} lines {r[3]:5d} -> {r[4]:5d}  vgpr {p['vgpr']:3d} -> {n['vgpr']:3d}  sgpr {p['sgpr']:3d} -> "
              f"{n['sgpr']:3d}  scratch {p['scratch']} -> {n['scratch']}  lds {p['lds']:5d} -> {n['lds']:5d}  {name}")
    for d in sorted(set(pkey) - kept):
        print(f"MISSING   a kernel of the parent has no dense form in the new tree: {d}")
    bad += len(set(pkey) - kept)
    print(f"{sum(r[0] != 'LENS' and r[2] is True for r in rows)} kernels of the parent identical, {bad} differing or missing, "
          f"{sum(r[0] == 'LENS' for r in rows)} ragged forms, {sum(r[2] is None for r in rows)} new kernels")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
