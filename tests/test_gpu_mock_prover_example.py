"""examples/mock_prover.py runs end to end on the device: the documentation example's failure, then simple-example checked and proved."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu


def test_mock_prover_example(capsys):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "mock_prover.py")
    spec = importlib.util.spec_from_file_location("mock_prover_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main([]) is True
    out = capsys.readouterr().out
    assert "Constraint 0 is not satisfied on row 0" in out and "advice[2]@+0 = 0x8" in out
    assert "MockProver is satisfied" in out and "accepted" in out
    assert mod.main(["--k", "6"]) is True
