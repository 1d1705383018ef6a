"""train.lr_factor, the learning-rate schedules of Stage1Trainer (train_x1_stage1_noiseinput.py:279-283, 513-521: diffusers'
get_scheduler), without a GPU.

Reference: transformers.optimization.get_scheduler driving a LambdaLR on a one-parameter SGD.  The reference's script imports
diffusers' get_scheduler, and diffusers is not installed here: that the two libraries' formulas for these six names agree
(same warm-up ramp, same decay expressions, same defaults num_cycles 0.5 / 1, power 1.0, lr_end 1e-7) is stated from
knowledge of both sources; no diffusers-written fixture pins it."""
import importlib

import pytest
import torch

NAMES = ("constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial")
TOTAL = 20
BASE_LR = 1e-3


@pytest.fixture(scope="module")
def TR():
    return importlib.import_module("video-gpt_amd.train")


def _reference(name, warmup, total, extra):
    from transformers.optimization import get_scheduler
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=BASE_LR)
    sched = get_scheduler(name, opt, num_warmup_steps=warmup, num_training_steps=total, scheduler_specific_kwargs=extra or None)
    lrs = []
    for _ in range(total + 6):
        lrs.append(sched.get_last_lr()[0])
        opt.step(); sched.step()
    return lrs


CASES = [(n, {}, {}) for n in NAMES] + [
    ("cosine", dict(num_cycles=1.5), dict(num_cycles=1.5)),
    ("cosine", dict(num_cycles=0.25), dict(num_cycles=0.25)),
    ("cosine_with_restarts", dict(num_cycles=3), dict(num_cycles=3)),
    ("polynomial", dict(power=2.0), dict(power=2.0)),
    ("polynomial", dict(power=0.5), dict(power=0.5)),
]


@pytest.mark.parametrize("warmup", [0, 3, 10])
@pytest.mark.parametrize("name,mine,theirs", CASES, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in m.items()) or 'defaults'}" for n, m, _ in CASES])
def test_lr_factor_is_get_schedulers_lambda(TR, name, mine, theirs, warmup):
    want = _reference(name, warmup, TOTAL, theirs)
    assert len(want) == TOTAL + 6                 # k = 0 .. total + 5
    for k, w in enumerate(want):
        got = BASE_LR * TR.lr_factor(name, k, warmup, TOTAL, mine.get("num_cycles"), mine.get("power", 1.0), BASE_LR)
        assert abs(got - w) <= 1e-12 * abs(w), (name, warmup, k, got, w)
        assert got >= 0.0
    assert len(set(want)) > 1 or name == "constant" or (name == "constant_with_warmup" and warmup == 0)


def test_lr_factor_refusals(TR):
    VgptError = importlib.import_module("video-gpt_amd.ops").VgptError
    for name in ("linear", "cosine", "cosine_with_restarts", "polynomial"):
        with pytest.raises(VgptError, match="lr_num_training_steps"):
            TR.lr_factor(name, 5, 2, None)
    for name in ("constant", "constant_with_warmup"):
        assert TR.lr_factor(name, 5, 2, None) == 1.0       # these two need no total
    with pytest.raises(VgptError) as e:
        TR.lr_factor("inverse_sqrt", 0, 0, 10)
    for name in NAMES:                                     # the message lists what is built
        assert name in str(e.value)
    assert TR.LR_SCHEDULERS == NAMES
