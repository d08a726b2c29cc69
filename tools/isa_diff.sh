#!/bin/bash
# Is the device code byte-for-byte what it was at another commit?  (development aid; needs hipcc, no GPU)
#   tools/isa_diff.sh <git-rev>                                      every kernel, matched by mangled name
#   tools/isa_diff.sh <git-rev> <name-fragment> [fragment-now]       one kernel (the third argument: its fragment in the current build when the mangled name changed)
# Compiles the revision's monorun_amd/csrc/ and include/ (git archive) and the working tree device-only for gfx950, then compares each kernel from
# its label through its .end_amdhsa_kernel descriptor, comments dropped and branch labels normalised (they carry the kernel's ordinal in the file).
# Used to land host-only changes, and changes meant for OTHER instantiations, without touching the tuned kernels: their register allocation
# reacts to almost anything.  Exit status 1 when a kernel present on both sides differs.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=$1; FRAG=$2; NEWFRAG=${3:-$2}
[ -n "$REV" ] || { sed -n '3,4p' "$0"; exit 2; }
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir -p "$T/old"
git -C "$ROOT" archive "$REV" monorun_amd/csrc include | tar -x -C "$T/old"
asm() { /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -I "$1/include" -S --cuda-device-only "$1/monorun_amd/csrc/monorun_pnp.hip" -o "$2" 2>/dev/null; }
asm "$T/old" "$T/old.s" & OLD=$!
asm "$ROOT" "$T/new.s"
wait $OLD
python3 - "$T/old.s" "$T/new.s" "$REV" "$FRAG" "$NEWFRAG" <<'EOF'
import re, sys
old_s, new_s, rev, frag, newfrag = sys.argv[1:]

def kernels(path):
    out, body = {}, []
    for raw in open(path):
        line = raw.split(';', 1)[0].rstrip()
        if not line.strip():
            continue
        if re.match(r'[^\s.][^\s:]*:$', line):          # a function's label starts its text
            body = []
        line = re.sub(r'\.(LBB|LCPI)\d+_', r'.\1_', line)
        body.append(re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', line))
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', line)
        if m:
            name = m.group(1)
        if line.strip() == '.end_amdhsa_kernel':
            out[name], body = body, []
    return out

old, new = kernels(old_s), kernels(new_s)
if frag:
    o = next((k for k in old if frag in k), None)
    n = next((k for k in new if newfrag in k), None)
    if o is None or n is None:
        sys.exit(f'no kernel matching {frag!r} at {rev} or {newfrag!r} now')
    diff = sum(a != b for a, b in zip(old[o], new[n])) + abs(len(old[o]) - len(new[n]))
    print(f'{o}: {len(old[o])} lines at {rev}, {len(new[n])} now, {diff} differing')
    sys.exit(1 if diff else 0)
both = sorted(set(old) & set(new))
differ = [k for k in both if old[k] != new[k]]
print(f'{len(old)} kernels at {rev}, {len(new)} now: {len(both) - len(differ)} identical, {len(differ)} differing')
for k in differ:
    print('  differs:', k)
for k in sorted(set(old) - set(new)):
    print(f'  only at {rev}:', k)
for k in sorted(set(new) - set(old)):
    print('  only now:', k)
sys.exit(1 if differ else 0)
EOF
