"""Check the DPP wait states of a kernel in the gfx950 assembly: every VGPR a DPP instruction reads
-- its DPP source, the old value of its destination (a bank-masked move keeps it in the masked-off
lanes; v_fmac accumulates into it) and its other sources -- must have been written at least two
wait states earlier (tools/ubench_dpp_fma.hip).  The compiler does not see
into the inline asm of GroupSys<HOPF>, so this reads the instruction stream it produced, in layout
order (a branch is one wait state; `s_nop N` is N + 1).  Usage, as tools/isa_loop_count.py:

    NNGP_ISA_S=/tmp/rk.s python tools/isa_dpp_waits.py [kernel-substring ...]   # default: every Hopf group kernel
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_loop_count import assembly  # noqa: E402

REG = re.compile(r'\bv(\d+)\b|\bv\[(\d+):(\d+)\]')


def regs(operand):
    out = set()
    for m in REG.finditer(operand):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def kernels(s, want):
    lines = s.split('\n')
    k = 0
    while k < len(lines):
        head = lines[k].split(';')[0].rstrip()
        if head.endswith(':') and not head.startswith('.') and any(w in head for w in want):
            end = next(j for j in range(k, len(lines)) if lines[j].startswith('.Lfunc_end'))
            yield head[:-1], lines[k + 1:end]
            k = end
        k += 1


def check(body):
    """(DPP instructions seen, violations) of one kernel"""
    recent = []   # (written VGPRs, text) of the last two wait states, newest last
    seen, bad = 0, []
    for raw in body:
        l = raw.split(';')[0].strip()
        if not l or l.endswith(':') or l.startswith('.'):
            continue
        op, _, rest = l.partition(' ')
        ops = [o.strip() for o in rest.split(',')]
        if op.endswith('_dpp'):
            seen += 1
            ops[-1] = ops[-1].split(' ')[0]   # drop the DPP controls behind the last operand
            read = set().union(*[regs(o) for o in ops])   # the destination's old value included
            for w, text in recent[-2:]:
                if w & read:
                    bad.append(f'{l}   <- {text}')
        if op == 's_nop':
            recent += [(set(), l)] * (int(ops[0], 0) + 1)
        else:
            recent.append((regs(ops[0]) if op.startswith('v_') and not op.startswith('v_cmp') else set(), l))
        recent = recent[-2:]
    return seen, bad


if __name__ == '__main__':
    s = assembly(fma=os.environ.get('NNGP_ISA_FMA') == '1')
    want = sys.argv[1:] or ['rk_group_kernelILi1E']
    fail = 0
    for name, body in kernels(s, want):
        seen, bad = check(body)
        print(f'{name}: {seen} DPP instructions, {len(bad)} read a VGPR written fewer than two wait states earlier')
        for b in bad:
            print('   ', b)
        fail += len(bad)
    sys.exit(1 if fail else 0)
