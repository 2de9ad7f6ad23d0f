#!/usr/bin/env python3
"""How k_step_roam's trip loop is laid out in the machine code: what stands between an entry's arrival and the next
gather, what each gather's shadow holds, and where the stop flag's load sits.

    python tools/roam_isa.py                       # disassembles ssrs_amd/libssrs_hip.so (llvm-objdump of the ROCm LLVM)
    python tools/roam_isa.py some/libssrs_hip.so
    python tools/roam_isa.py tracks.s              # a listing: hipcc <flags of csrc/build.py> -S --cuda-device-only

The trip loop is found without reading a single vector instruction: it is the SHORTEST cycle of the kernel's control
flow graph through the stop flag's load (the one `global_load_dword ... sc1`), counted in instructions.  Every rare
continuation -- a visit outside the window, the single-move sequence, the stepping wave's own Philox when a record is
not there -- only adds instructions, so the shortest cycle is the path a settled wave runs.  On it the tool looks for
`s_waitcnt` with a vmcnt operand, `global_load_dwordx4` (the pair-table gathers), the flag load, `ds_*` and branches.

Counts are instructions strictly between the two named ones; `s_waitcnt` and `s_nop` are not counted (they issue
nothing).  The trip boundary is the gather-to-wait stretch that holds the loop's backward branch.
"""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, 'ssrs_amd', 'libssrs_hip.so')
ARCH = 'gfx950'
BUNDLE_MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def find_objdump():
    """llvm-objdump of the ROCm LLVM, or None."""
    dirs = []
    for var in ('ROCM_PATH', 'ROCM_HOME', 'HIP_PATH'):
        if os.environ.get(var):
            dirs.append(os.path.join(os.environ[var], 'llvm', 'bin'))
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    dirs.append(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), 'llvm', 'bin'))
    dirs.append('/opt/rocm/llvm/bin')
    for d in dirs:
        p = os.path.join(d, 'llvm-objdump')
        if os.access(p, os.X_OK):
            return p
    return shutil.which('llvm-objdump')


# ---------------------------------------------------------------- ELF, just enough of it
class Elf:
    def __init__(self, data):
        if data[:4] != b'\x7fELF' or data[4] != 2 or data[5] != 1:
            raise ValueError('not a little-endian ELF64 image')
        self.data = data
        shoff, = struct.unpack_from('<Q', data, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from('<HHH', data, 0x3A)
        raw = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
        stroff, strsize = raw[shstrndx][4], raw[shstrndx][5]
        strtab = data[stroff:stroff + strsize]
        self.sections = []
        for name, typ, _flags, addr, off, size, link, _info, _align, entsize in raw:
            self.sections.append(dict(name=strtab[name:strtab.index(b'\0', name)].decode(), type=typ, addr=addr,
                                      off=off, size=size, link=link, entsize=entsize))

    def section(self, name):
        for s in self.sections:
            if s['name'] == name:
                return s
        return None

    def symbols(self):
        out = {}
        for s in self.sections:
            if s['type'] != 2:                                           # SHT_SYMTAB
                continue
            st = self.sections[s['link']]
            names = self.data[st['off']:st['off'] + st['size']]
            for i in range(s['size'] // 24):
                name, _info, _other, _shndx, value, size = struct.unpack_from('<IBBHQQ', self.data, s['off'] + 24 * i)
                out[names[name:names.index(b'\0', name)].decode()] = (value, size)
        return out

    def read(self, addr, n):
        for s in self.sections:
            if s['type'] != 8 and s['addr'] <= addr and addr + n <= s['addr'] + s['size']:      # (not SHT_NOBITS)
                o = s['off'] + addr - s['addr']
                return self.data[o:o + n]
        raise ValueError(f'address {addr:#x} is in no section')


def code_objects(lib_path):
    """The gfx950 code objects bundled into a host library (one per translation unit)."""
    data = open(lib_path, 'rb').read()
    if data[:4] == b'\x7fELF' and struct.unpack_from('<H', data, 0x12)[0] == 224:       # EM_AMDGPU: a code object itself
        return [data]
    sec = Elf(data).section('.hip_fatbin')
    if sec is None:
        raise ValueError(f'{lib_path}: no .hip_fatbin section')
    blob = data[sec['off']:sec['off'] + sec['size']]
    out = []
    at = blob.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from('<Q', blob, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from('<QQQ', blob, p)
            ident = blob[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if ARCH in ident and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(BUNDLE_MAGIC, at + len(BUNDLE_MAGIC))
    if not out:
        raise ValueError(f'{lib_path}: no uncompressed {ARCH} code object in .hip_fatbin')
    return out


# ---------------------------------------------------------------- instructions and their successors
class Insn:
    __slots__ = ('mn', 'ops', 'target', 'key')

    def __init__(self, mn, ops, target, key):
        self.mn, self.ops, self.target, self.key = mn, ops, target, key      # target: a label / an address, or None


def is_branch(mn):
    return mn == 's_branch' or mn.startswith('s_cbranch')


def demangled(sym):
    m = re.match(r'_ZN4ssrs11k_step_roamILb([01])ELi(\d+)ELb([01])EEE', sym)
    return f'k_step_roam<{"true" if m.group(1) == "1" else "false"}, {m.group(2)}, {"true" if m.group(3) == "1" else "false"}>' if m else sym


def parse_listing(path):
    """{kernel: (instructions, label -> index, ScratchSize, LDSByteSize)} of a -S listing."""
    out = {}
    cur = None
    with open(path, errors='replace') as f:
        for line in f:
            m = re.match(r'(_ZN4ssrs11k_step_roam\w+):', line)
            if m:
                cur = dict(name=m.group(1), insns=[], labels={}, scratch=None, lds=None)
                continue
            if cur is None:
                continue
            m = re.match(r'; (ScratchSize|LDSByteSize): (\d+)', line)
            if m:
                cur['scratch' if m.group(1) == 'ScratchSize' else 'lds'] = int(m.group(2))
                if cur['scratch'] is not None and cur['lds'] is not None:
                    out[demangled(cur['name'])] = (cur['insns'], cur['labels'], cur['scratch'], cur['lds'])
                    cur = None
                continue
            m = re.match(r'([.\w$]+):', line)
            if m:
                cur['labels'][m.group(1)] = len(cur['insns'])
                continue
            if not line.startswith('\t'):
                continue
            text = line.split(';')[0].strip()
            if not text or text.startswith('.'):
                continue
            mn, _, ops = text.partition(' ')
            ops = ops.strip()
            cur['insns'].append(Insn(mn, ops, ops.split(',')[0].strip() if is_branch(mn) else None, len(cur['insns'])))
    return out


def parse_library(lib_path, objdump):
    """The same of a built library, through llvm-objdump."""
    out = {}
    for co in code_objects(lib_path):
        elf = Elf(co)
        syms = elf.symbols()
        kernels = [s for s in syms if s.startswith('_ZN4ssrs11k_step_roam') and not s.endswith('.kd')]
        if not kernels:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            cop = os.path.join(tmp, 'tracks.co')
            with open(cop, 'wb') as f:
                f.write(co)
            for k in kernels:
                txt = subprocess.run([objdump, '-d', f'--disassemble-symbols={k}', cop], check=True,
                                     stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True).stdout
                insns, labels = [], {}
                for line in txt.splitlines():
                    m = re.match(r'\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):((?:\s+[0-9A-Fa-f]{8})+)', line)
                    if not m:
                        continue
                    mn, ops, addr = m.group(1), m.group(2), int(m.group(3), 16)
                    target = None
                    if is_branch(mn):
                        imm = int(m.group(4).split()[0], 16) & 0xFFFF                      # SOPP: simm16 in dwords
                        target = addr + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)
                    labels[addr] = len(insns)
                    insns.append(Insn(mn, ops, target, addr))
                kd = syms.get(k + '.kd')
                lds = scratch = None
                if kd:
                    lds, scratch = struct.unpack('<II', elf.read(kd[0], 8))      # group / private segment fixed sizes
                out[demangled(k)] = (insns, labels, scratch, lds)
    return out


def hot_cycle(insns, labels):
    """Indices of the shortest cycle through the stop flag's load, beginning behind it; None without such a load."""
    flags = [i for i, x in enumerate(insns) if x.mn.startswith('global_load_dword') and not x.mn.startswith('global_load_dwordx')
             and re.search(r'\bsc1\b', x.ops)]
    best = None
    for f in flags:
        prev = {f: None}
        q = deque([f])
        found = None
        while q and found is None:
            i = q.popleft()
            x = insns[i]
            succ = []
            if is_branch(x.mn) and x.target in labels:
                succ.append(labels[x.target])
            if x.mn not in ('s_branch', 's_endpgm', 's_setpc_b64') and i + 1 < len(insns):
                succ.append(i + 1)
            for j in succ:
                if j == f:
                    found = i
                    break
                if j not in prev:
                    prev[j] = i
                    q.append(j)
        if found is None:
            continue
        path = []
        i = found
        while i is not None:
            path.append(i)
            i = prev[i]
        path.reverse()                                                          # f, ..., found (whose successor is f)
        if best is None or len(path) < len(best):
            best = path
    return best


def counted(x):
    return x.mn not in ('s_waitcnt', 's_nop')


def vmcnt_of(x):
    if x.mn != 's_waitcnt':
        return None
    m = re.search(r'vmcnt\((\d+)\)', x.ops)
    if m:
        return int(m.group(1))
    m = re.fullmatch(r'(0x[0-9a-fA-F]+|\d+)', x.ops)                         # a raw immediate: vmcnt in bits 3:0 and 15:14
    if m:
        v = int(m.group(1), 0)
        v = (v & 0xF) | ((v >> 14) & 0x3) << 4
        return None if v == 63 else v
    return None


def analyse(insns, labels):
    path = hot_cycle(insns, labels)
    if path is None:
        return None
    n = len(path)
    seq = [insns[i] for i in path]                                               # seq[0] is the flag load
    # the backward branch of the loop: the step of the cycle that jumps furthest back
    back = max(range(n), key=lambda p: path[p] - path[(p + 1) % n])
    start = (back + 1) % n                                                       # the loop header
    order = [(start + p) % n for p in range(n)]                                  # positions in trip order
    seq = [seq[p] for p in order]
    flag_at = order.index(0)
    gathers = [p for p, x in enumerate(seq) if x.mn == 'global_load_dwordx4']
    waits = [p for p, x in enumerate(seq) if vmcnt_of(x) is not None]

    def between(p, q):                                                          # strictly between, cyclically
        c, r = 0, (p + 1) % n
        while r != q:
            c += counted(seq[r])
            r = (r + 1) % n
        return c

    def next_of(p, where):
        r = (p + 1) % n
        while r not in where:
            r = (r + 1) % n
        return r

    pairs = []
    for g in gathers:
        w_after = next_of(g, waits)
        w_before = g
        # the wait for this gather's entry: the first vmcnt wait behind the previous gather
        g_prev = gathers[gathers.index(g) - 1]
        w_before = next_of(g_prev, waits)
        crosses = w_after < g                                                    # wrapped round the loop's backward branch
        pairs.append(dict(wait_vmcnt=vmcnt_of(seq[w_before]), wait_to_gather=between(w_before, g),
                          gather_to_wait=between(g, w_after), boundary=crosses,
                          ds=[x.mn for x in (seq[(g + 1 + d) % n] for d in range((w_after - g - 1) % n)) if x.mn.startswith('ds_')],
                          branches=sum(is_branch(x.mn) for x in (seq[(g + 1 + d) % n] for d in range((w_after - g - 1) % n)))))
    return dict(cycle=sum(counted(x) for x in seq), pairs=pairs, waits=[vmcnt_of(seq[p]) for p in waits],
                flag_to_wait=between(flag_at, next_of(flag_at, waits)),
                flag_behind_gather=between(max([g for g in gathers if g < flag_at] or [gathers[-1]]), flag_at) if gathers else None)


def report(path=None):
    """{kernel: analysis + ScratchSize + LDSByteSize} of a library (default: the built one) or a -S listing."""
    path = path or DEFAULT_LIB
    if path.endswith('.s') or path.endswith('.S'):
        parsed = parse_listing(path)
    else:
        objdump = find_objdump()
        if objdump is None:
            raise RuntimeError('llvm-objdump of the ROCm LLVM not found')
        parsed = parse_library(path, objdump)
    out = {}
    for name, (insns, labels, scratch, lds) in sorted(parsed.items()):
        r = analyse(insns, labels) or {}
        r.update(scratch=scratch, lds=lds, instructions=len(insns))
        out[name] = r
    return out


def main(argv):
    rep = report(argv[1] if len(argv) > 1 else None)
    if not rep:
        print('no k_step_roam instantiation found')
        return 1
    for name, r in rep.items():
        print(f'{name}: ScratchSize {r["scratch"]}, LDSByteSize {r["lds"]}, {r["instructions"]} instructions')
        if 'pairs' not in r:
            print('  no stop-flag load (sc1) on a cycle: trip loop not found')
            continue
        print(f'  trip: {r["cycle"]} instructions on the settled path; vmcnt waits on it: {r["waits"]}')
        inside = [p['gather_to_wait'] for p in r['pairs'] if not p['boundary']]
        for q, p in enumerate(r['pairs'], 1):
            where = 'ACROSS THE TRIP BOUNDARY' if p['boundary'] else 'inside the trip'
            print(f'  pair {q}: wait vmcnt({p["wait_vmcnt"]}) -> gather {p["wait_to_gather"]:3d};  gather -> next wait '
                  f'{p["gather_to_wait"]:3d} ({where}; {p["branches"]} branches; {" ".join(p["ds"]) or "no ds"})')
        for p in r['pairs']:
            if p['boundary'] and inside:
                print(f'  boundary - largest inside: {p["gather_to_wait"] - max(inside):+d}')
        print(f'  flag load: {r["flag_behind_gather"]} behind a gather, {r["flag_to_wait"]} before the next vmcnt wait')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
