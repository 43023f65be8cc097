#!/bin/bash
# Are two trees' kernels the same machine code?  Builds every csrc/*.hip of git revision REV in a
# worktree with the library's own flags and compares, per translation unit, the gfx950 code
# object's .text and .rodata (kernel code + descriptors) with the current in-tree build
# (beast_tokenizer_amd/csrc/build).  The host wrappers and the fat binary's bundle metadata
# (which carries paths) are not compared.  A unit that differs is disassembled on both sides and
# listed per kernel symbol: same / DIFFERENT by instruction text alone (addresses, encodings and
# branch targets stripped), with the VGPR / SGPR / LDS / scratch of both builds beside a kernel
# that differs.                                bash tools/codeobj_compare.sh REV
set -eu
REV="$1"; R="$(cd "$(dirname "$0")/.." && pwd)"; W=/tmp/codeobj_wt_$$; O=/tmp/codeobj_o_$$
B=/opt/rocm/lib/llvm/bin
git -C "$R" worktree add -q "$W" "$REV"
mkdir -p "$O"
(cd "$W" && python3 - "$O" <<'PY'
import os, subprocess, sys
sys.path.insert(0, os.getcwd())
from beast_tokenizer_amd import _build
for src in _build._sources():
    subprocess.run([_build._hipcc(), *_build.CXXFLAGS, *_build.FILE_FLAGS.get(os.path.basename(src), []), "-c", src,
                    "-o", os.path.join(sys.argv[1], os.path.basename(src)[:-4] + ".o")], check=True)
PY
)
for o in "$O"/*.o; do
  f=$(basename "$o" .o); n="$R/beast_tokenizer_amd/csrc/build/$f.o"
  [ -f "$n" ] || { echo "$f: not in the current build"; continue; }
  r=""
  for w in old new; do
    src=$([ $w = old ] && echo "$o" || echo "$n")
    $B/llvm-objcopy --dump-section=.hip_fatbin="$O/$w.fatbin" "$src" 2>/dev/null || { r=" no device code"; break; }
    $B/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$O/$w.fatbin" --output="$O/$w.co" --unbundle
    for s in .text .rodata; do $B/llvm-objcopy --dump-section=$s="$O/$w$s" "$O/$w.co"; done
  done
  if [ -z "$r" ]; then for s in .text .rodata; do cmp -s "$O/old$s" "$O/new$s" && r="$r $s same" || r="$r $s DIFFERENT"; done; fi
  echo "$f:$r"
  case "$r" in *DIFFERENT*) python3 - "$B" "$O/old.co" "$O/new.co" <<'PY'
import re, subprocess, sys
B, old, new = sys.argv[1:4]


def kernels(co):
    """symbol -> its instructions as text: no addresses, no encodings, no branch targets"""
    out, cur = {}, None
    dis = subprocess.run([B + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            ins = line.split("//")[0].strip()
            cur.append(ins.split()[0] if re.match(r"s_c?branch", ins) else ins)
    return out


def resources(co):
    """kernel symbol -> the descriptor fields that matter, from the code object's metadata note"""
    note = subprocess.run([B + "/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", note)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\S+)",
                            blk))
        res[f.get("name")] = "vgpr %s sgpr %s lds %s scratch %s" % (
            f.get("vgpr_count"), f.get("sgpr_count"), f.get("group_segment_fixed_size"),
            f.get("private_segment_fixed_size"))
    return res


ko, kn, ro, rn = kernels(old), kernels(new), resources(old), resources(new)
names = sorted(set(ko) | set(kn))
for k in names:
    if k not in ko or k not in kn:
        print("    %s: only in the %s build" % (k, "new" if k in kn else "old"))
    elif ko[k] == kn[k]:
        print("    %s: same" % k)
    else:
        print("    %s: DIFFERENT (%d -> %d instructions; old %s; new %s)" % (k, len(ko[k]), len(kn[k]), ro.get(k), rn.get(k)))
print("    %d of %d kernels same" % (sum(1 for k in names if ko.get(k) == kn.get(k)), len(names)))
PY
  ;; esac
done
git -C "$R" worktree remove --force "$W"; rm -rf "$O"
