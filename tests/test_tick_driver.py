"""CPU-only tests of the tick loop's bookkeeping (engine.TickDriver, engine.tick_until) and of the small helpers beside it
(module_of, default_device, close_all): a fake tick that appends to a list, stub engines, no device."""
import pytest
import torch

from alphazero_openspiel_amd import engine as E


class _Engine:
    def __init__(self, name, log=None):
        self.name, self.log = name, log if log is not None else []

    def progress(self):
        return {"engine": self.name}

    def close(self):
        self.log.append(self.name)


def test_eager_run_calls_tick_n_times_and_counts_them():
    calls = []
    drv = E.TickDriver(None, lambda: calls.append(len(calls)))
    assert drv.ticks == 0 and drv.graph is None
    drv.run(5)
    assert calls == [0, 1, 2, 3, 4] and drv.ticks == 5
    drv.run(1)
    drv.run(16)
    assert len(calls) == 22 and drv.ticks == 22


def test_tick_until_polls_once_per_batch_and_returns_on_the_batch_that_finishes():
    calls, polls = [], []
    drv = E.TickDriver(None, lambda: calls.append(1))

    def done():
        polls.append(drv.ticks)
        return len(polls) == 3

    E.tick_until(drv, 4, done, None, "arena")
    assert polls == [4, 8, 12] and len(calls) == 12 and drv.ticks == 12
    E.tick_until(drv, 4, lambda: True, 1, "arena")  # done on the first batch: the limit is not looked at
    assert drv.ticks == 16


def test_tick_until_raises_the_callers_message_once_the_limit_is_reached():
    polls = []
    drv = E.TickDriver(None, lambda: None)
    with pytest.raises(E.EngineError) as err:
        E.tick_until(drv, 4, lambda: polls.append(drv.ticks), 10, "duel", _Engine("a"), _Engine("b"))
    assert polls == [4, 8, 12] and drv.ticks == 12  # 4, 8 < 10: go on; 12 >= 10: raise
    assert str(err.value) == "duel did not finish within 10 ticks: {'engine': 'a'} / {'engine': 'b'}"
    with pytest.raises(E.EngineError) as err:
        E.tick_until(E.TickDriver(None, lambda: None), 16, lambda: False, 16, "self-play", _Engine("e"))
    assert str(err.value) == "self-play did not finish within 16 ticks: {'engine': 'e'}"


def test_module_of_accepts_a_module_or_its_bound_predict_only():
    class Net(torch.nn.Linear):
        def predict(self, state):
            return None

        def other(self, state):
            return None

    net = Net(2, 2)
    assert E.module_of(net) is net and E.module_of(net.predict) is net
    assert E.module_of(net.other) is None and E.module_of(lambda s: None) is None and E.module_of(None) is None


def test_default_device_is_the_current_hip_device_unless_the_net_is_on_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    current = torch.device("cuda", 3)
    assert E.default_device(None) == current and E.default_device(lambda s: None) == current
    assert E.default_device(torch.nn.Linear(2, 2)) == current                # parameters on the CPU
    assert E.default_device(torch.nn.ReLU()) == current                      # a module without parameters

    class _Par:
        is_cuda, device = True, torch.device("cuda", 1)

    class OnGpu(torch.nn.Module):
        def parameters(self, recurse=True):
            return iter([_Par()])

    assert E.default_device(OnGpu()) == torch.device("cuda", 1)


def test_close_all_closes_what_has_a_close_in_the_order_given():
    log = []
    E.close_all(_Engine("a", log), None, object(), _Engine("b", log))
    assert log == ["a", "b"]
    E.close_all()
    assert log == ["a", "b"]
