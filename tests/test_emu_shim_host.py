"""The two host shims of tests/emu held to their own contract ("The host shims"): toy kernels, tests/emu/selftest.cpp, under the
sequential shim -- plain, under AddressSanitizer and UBSan, and with waves of one lane -- and under the threaded one.  The host tests of
fifteen kernel families rely on what is shown here: a ballot's mask, a barrier, the workgroup's vote, the counters, and above all that a
collective point which only some lanes reach ends the program with exit code 4."""
import subprocess

import pytest

import emu_build


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    seq = emu_build.build(tmp_path_factory, "emu", (), {"selftest": (), "selftest_san": emu_build.SAN, "selftest_alone": ("-DEMU_LANES_ALONE",)}, source="selftest.cpp")
    thr = emu_build.build(tmp_path_factory, "emu", (), {"selftest": ()}, flags=("-DEMU_THREADS",), threads=True, source="selftest.cpp")
    return seq, thr


def run(where, exe, case):
    return subprocess.run(["./" + exe, case], cwd=where, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("exe", ["selftest", "selftest_san"])
@pytest.mark.parametrize("case", ["ballots_64", "ballots_256", "barrier_64", "barrier_256", "votes_64", "votes_256", "any"])
def test_sequential_shim(programs, exe, case):
    """ballots_*: pred = lane % 3 == 0 gives every lane 0x9249249249249249 twice, blockIdx, gridDim and blockDim read as launched;
    barrier_*: lane l stores l, passes the barrier and reads slot n - 1 - l, in static and in dynamic shared memory (exactly the bytes
    asked for: selftest_san would see an overrun); votes_*: one lane's yes is the workgroup's, a wave without a yes answers no; any: the wave's
    answer, not the lane's.  Each checks the counters its kernel implies."""
    r = run(programs[0], exe, case)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("case,message", [
    ("lane_leaves_before_a_ballot", "a ballot reached by some lanes of its wave only"),       # lane 5 of 64
    ("lane_leaves_before_a_barrier", "a workgroup's vote or barrier reached by some of its lanes only"),  # lane 70 of 256
    ("wave_alone_at_a_vote", "a workgroup's vote or barrier reached by some of its lanes only"),  # wave 1 takes a vote that wave 0 does not
    ("waves_disagree", "the waves of a workgroup disagree about its next vote"),              # wave 1 has taken a vote of its own before
])
def test_sequential_shim_ends_a_defect_with_exit_code_4(programs, case, message):
    r = run(programs[0], "selftest", case)
    assert r.returncode == 4 and r.stderr.strip() == message and r.stdout == "", (r.returncode, r.stdout, r.stderr[-2000:])


def test_lanes_alone_answer_for_themselves(programs):
    """-DEMU_LANES_ALONE leaves FDH_MSDF_ANY to the kernel's own fallback: the lane's own word"""
    r = run(programs[0], "selftest_alone", "any")
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr[-2000:])


def test_threaded_shim(programs):
    """__shfl_xor and __shfl_up across a wave, a ballot inside a branch only wave 1 takes, a barrier, and atomicAdd from every thread of a
    grid of 4: 256 x 4"""
    r = run(programs[1], "selftest", "threads")
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr[-2000:])
