"""bench.py's command line: a plain run does only what the headline figure needs; --full adds the check, the
host-pointer call, the CPU baseline and the irregular stand-in, and the explicit switches still override."""
import pytest

import bench


def test_plain_run_is_lean():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (a.full, a.check, a.host_exec, a.cpu_baseline, a.also) == (False, 0, 0, False, False)
    assert a.dump_outputs is None and not a.sweep_variants


def test_full_runs_every_leg():
    a = bench.parse_args(["--full"])
    assert (a.full, a.check, a.host_exec, a.cpu_baseline, a.also) == (True, 1, 1, True, True)


@pytest.mark.parametrize("argv, want", [
    (["--full", "--no-cpu-baseline"], (1, 1, False, True)),
    (["--full", "--no-also", "--host-exec", "0"], (1, 0, True, False)),
    (["--full", "--check", "0"], (0, 1, True, True)),
    (["--check", "1"], (1, 0, False, False)),
    (["--host-exec", "1", "--no-cpu-baseline"], (0, 1, False, False)),
])
def test_explicit_switches_override(argv, want):
    a = bench.parse_args(argv)
    assert (a.check, a.host_exec, a.cpu_baseline, a.also) == want


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
