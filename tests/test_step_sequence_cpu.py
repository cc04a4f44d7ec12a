"""The order of everything a training-step driver enqueues, against the record made before engine.EagerStep existed.

profiles/step_sequence_equivalence.py drives train_one_step / train_one_step_trajectory, JointStep, GraphedStep (construction, then
launch / finish on the mocked graphs), GraphedJointStep and the trainers' StepRunner with recording stand-ins (optimizer, step function,
torch.distributed, torch.cuda's stream / event / graph surface, lib.load()) around the real FlatDataParallel;
profiles/step_sequence_equivalence.json is its output at the commit before the refactor.  Equality is exact, with two exceptions that
`differences()` encodes: in the joint step the trajectory optimizer's zero_grad may sit elsewhere in the interleaved order (each model's
own events are identical), and GraphedStep's warm-up may hold additional arm(True) events."""
import copy
import importlib.util
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def SE():
    spec = importlib.util.spec_from_file_location("step_sequence_equivalence",
                                                  os.path.join(REPO, "profiles", "step_sequence_equivalence.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(REPO, "profiles", "step_sequence_equivalence.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def now(SE):
    return SE.record(REPO)


def test_every_listed_case_is_recorded(SE, recorded):
    names = set(recorded)
    assert names == set(SE.cases())
    for which in ("train_one_step", "train_one_step_trajectory"):
        for mode in ("no ddp", "world 8 overlapped", "world 8 one shot"):
            for acc in (1, 3):
                case = recorded["%s: %s, accumulate %d" % (which, mode, acc)]
                assert [e[2] for e in case["log"] if e[1] == "step_id"] == list(range(6))
    assert set(SE.JOINT_CASES) <= names
    for world in (1, 8):
        for prefetch in ("off", "on"):
            assert "GraphedStep: world %d, prefetch %s" % (world, prefetch) in names
    raised = recorded["GraphedStep: world 8, prefetch on, the step function raises before the split point"]["log"]
    assert raised[-1][1] == "raised"
    # no capture left open, the prefetch stream joined before the capture ended
    assert [e[1] for e in raised].count("capture begin") == [e[1] for e in raised].count("capture end") == 1
    assert [e[1:] for e in raised[-3:-1]] == [["wait_stream", "main", "stream1"], ["capture end", "graph0"]]
    for family in ("keypose", "trajectory"):
        for tail in ("accumulate 1", "accumulate 2", "eval mode"):
            case = recorded["StepRunner: %s, %s" % (family, tail)]
            assert "".join(e[3] for e in case["log"] if e[1] == "step_id") == "AAABABB"
    assert recorded["StepRunner: keypose, accumulate 1"]["replays"] == 5        # A A A B A B B: all but each shape's first sighting
    assert recorded["StepRunner: keypose, accumulate 2"]["replays"] == recorded["StepRunner: keypose, eval mode"]["replays"] == 0


def test_step_call_sequences_equal_the_record(SE, recorded, now):
    bad = SE.differences(recorded, now)
    assert not bad, "\n".join(bad)


def test_the_comparison_is_exact_outside_its_two_exceptions(SE, recorded):
    """differences() itself: any other change is reported, the two stated ones are not"""
    def changed(name, edit):
        other = copy.deepcopy(recorded)
        edit(other[name]["log"])
        return SE.differences(recorded, other)

    joint, graphed = SE.JOINT_CASES[1], "GraphedStep: world 8, prefetch on"
    log = recorded[joint]["log"]
    i, k = log.index(["tr", "zero_grad"]), log.index(["tr", "arm", True])
    assert changed(joint, lambda l: l.insert(k - 1, l.pop(i))) == []                 # the trajectory zero_grad, later
    assert changed(joint, lambda l: l.insert(k, l.pop(log.index(["kp", "zero_grad"]))))   # the keypose one may not move
    assert changed(joint, lambda l: l.pop(i))                                        # ... and the trajectory one may not vanish
    assert changed(joint, lambda l: l.insert(len(l) - 1, l.pop(i)))                  # ... nor run after its own step
    sync = recorded[graphed]["log"].index(["step", "synchronize"])
    assert changed(graphed, lambda l: l.insert(2, ["step", "arm", True])) == []      # warm-up: an additional arm(True)
    assert changed(graphed, lambda l: l.insert(sync + 2, ["step", "arm", True]))     # not after the warm-up
    assert changed(graphed, lambda l: l.insert(2, ["step", "arm", False]))           # and nothing else
    assert changed(graphed, lambda l: l.insert(2, ["step", "zero_grad"]))
    swap = lambda l: l.__setitem__(slice(sync + 1, sync + 3), [l[sync + 2], l[sync + 1]])
    assert changed(graphed, swap)
