"""Cross-check of the CPU oracle against the upstream caller itself, on inputs that are NOT in the other fixtures.

The upstream caller's results on these inputs are stored in tests/golden/reference_live.json, so the check runs anywhere;
`python tests/test_reference_live.py` re-derives that file where the upstream tree is importable (tests/golden/_ref_import.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'reference_live.json')
CASES = [('(AGC)', 16, 9001), ('(CTG)AA(CCG)', 18, 9002)]

_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1] + '/tests/golden'); sys.path.insert(0, sys.argv[1])
import numpy as np
from _ref_import import import_reference
from warpstr_amd import synth
ns = import_reference()
pattern, fl, seed = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
locus = synth.make_locus(pattern, fl, seed)
sigs, revs, _ = synth.batch(locus, 3, (700, 1100), seed + 1, lo=3, hi=12)
rev_seq = locus.left_r + ns.wrapper.CallerWrapper.reverse_uniq_sequence(pattern) + locus.right_r
stas = {False: ns.automata.StateAutomata(locus.left_t + pattern + locus.right_t), True: ns.automata.StateAutomata(rev_seq)}
out = []
for s, r in zip(sigs, revs):
    sta = stas[r]
    w = ns.caller.WarpSTR(fl, sta.states, sta.endstate, sta.mask, None, r, 'x')
    try:
        res = w.run(s)
        out.append(dict(ok=True, len1=len(res.seq), len2=len(res.resc_seq), cost1=float(res.cost), cost2=float(res.resc_cost)))
    except Exception as e:
        out.append(dict(ok=False, err=type(e).__name__))
print('RESULT ' + json.dumps(out))
'''


def _upstream(pattern, fl, seed):
    """The upstream caller on one case, in a child process (it parses its configuration from argv at import time)."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    p = subprocess.run([sys.executable, '-c', _CHILD, ROOT, pattern, str(fl), str(seed)], capture_output=True, text=True,
                       env=env, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
    assert line, p.stderr[-2000:]
    return json.loads(line[0][7:])


@pytest.mark.parametrize('pattern,fl,seed', CASES)
def test_oracle_agrees_with_live_reference(pattern, fl, seed):
    with open(FIXTURE) as f:
        ref = json.load(f)['cases'][f'{pattern}|{fl}|{seed}']
    sys.path.insert(0, ROOT)
    from oracle import oracle
    from warpstr_amd import synth
    locus = synth.make_locus(pattern, fl, seed)
    sigs, revs, _ = synth.batch(locus, 3, (700, 1100), seed + 1, lo=3, hi=12)
    assert len(ref) == len(sigs) == 3
    oa = {False: oracle.Automaton.from_table(locus.template, fl), True: oracle.Automaton.from_table(locus.reverse, fl)}
    for s, r, exp in zip(sigs, revs, ref):
        o = oracle.call_read(oa[r], s)
        if exp['ok']:
            assert o.status == 0 and (o.len1, o.len2) == (exp['len1'], exp['len2'])
            assert abs(o.cost1 - exp['cost1']) <= 1e-12 * abs(exp['cost1'])
            assert abs(o.cost2 - exp['cost2']) <= 1e-12 * abs(exp['cost2'])
        else:
            assert o.status != 0


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from _ref_import import reference_available
    if not reference_available():
        raise SystemExit('the upstream tree is not importable here (tests/golden/_ref_import.py)')
    with open(FIXTURE) as f:
        about = json.load(f)['about']
    cases = {f'{p}|{fl}|{seed}': _upstream(p, fl, seed) for p, fl, seed in CASES}
    with open(FIXTURE, 'w') as f:
        json.dump({'about': about, 'cases': cases}, f, indent=1)
        f.write('\n')
