"""GPU: every level-1 kernel row of dbgk_l1_form.h's lists runs under its own name and equals the oracle.  The cases are
tests/l1_form_cases.py's (one per row; tests/test_l1_form_cpu.py pins their plans on the CPU); tests/l1_forms_gpu_steps.py runs them,
one handle per step, each step a child process under its own time limit: a fault in a row that never ran before ends that step and
nothing after it.  What "by name" buys: if the selection changes -- a later level-1 change, a transposed flag, a threshold moved --
Graph.l1_forms() no longer equals the case's launches although the results are still right; if a row computes something wrong, the
comparison with the oracle fails and names the row."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import l1_form_cases as LC  # noqa: E402
import l1_forms_gpu_steps as S  # noqa: E402


def test_steps_run_every_selectable_case_once():
    """(no GPU needed) the steps partition the cases; no step has more than 16 rows; a limit is five times the measured time, at least 60 s"""
    cases = LC.cases()
    ran = [c.row for step in S.STEPS for c in S.cases_of(step)]
    assert sorted(ran) == sorted(set(cases) - set(LC.UNSELECTABLE))
    assert {S.step_of(c) for c in cases.values()} == set(S.STEPS)
    for step, (measured, limit) in S.STEPS.items():
        assert 1 <= len(S.cases_of(step)) <= 16 and limit >= 60 and limit >= 5 * measured and measured <= 30, step


@pytest.mark.gpu
@pytest.mark.parametrize("step", sorted(S.STEPS))
def test_rows_run_by_name_and_equal_the_oracle(step):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "l1_forms_gpu_steps.py"), step], capture_output=True, text=True,
                       timeout=S.STEPS[step][1], cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["step"] == step and res["rows"] == len(S.cases_of(step))
