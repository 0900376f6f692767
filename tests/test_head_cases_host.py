"""The nets of the head tests (head_cases.py) without a GPU: that net_cases.trained_head gives every case net what its docstring
promises, measured on the float64 forward alone, and that the isolated float64 reference of the head (net_cases.head_fp64 with
net_cases.head_weights), fed the float64 tower output, reproduces the float64 Net - its K indexing (position * stride + channel)
and its restatement of the weight rounding of every device path are right."""
import copy

import numpy as np
import pytest
import torch

import head_cases as hc
from net_cases import head_fp64, head_weights, tower_fp64

KEYS = list(hc.NETS)


@pytest.mark.parametrize("key", KEYS)
def test_trained_head_properties(key):
    q = hc.head_properties(key)
    print(key, {k: v for k, v in q.items() if k not in ("p", "v", "logits")})
    # a peaked softmax next to a flat one: logits that span tens of units, priors from about 1 down to below 1e-12
    assert q["span_max"] > 40 and q["wide_span"] >= 0.05
    assert q["peaked"] >= 0.05 and q["min_prior"] < 1e-12
    assert q["uniform"] >= 0.03
    # the value logit saturates tanh on some boards and stays in its linear part on others
    assert q["v_sat"] >= 0.05 and q["v_lin"] >= 0.03
    # biases: distinct, of order 1, none zero
    assert q["bias_distinct"] and 0.25 <= q["bias_min"] and q["bias_max"] <= 1.5
    # weights whose fp16 hi half is subnormal, and whose f32x lo half (x 2048) is subnormal too; none is exactly zero
    assert q["w_sub"] >= 0.02 and q["w_sub_lo"] >= 0.005 and q["w_zero"] == 0.0
    # nothing leaves fp16's range in the net or float32's in the logits
    assert q["top"] < 65504.0 and q["logit_max"] < 65504.0
    assert np.isfinite(q["logits"].astype(np.float32)).all()


@pytest.mark.parametrize("key", KEYS)
def test_isolated_head_reference_reproduces_the_float64_net(key):
    net, A = hc.net(key), hc.NETS[key][1]
    ob = hc.obs(key)[:hc.N_E2E]
    with torch.no_grad():
        p64, v64 = copy.deepcopy(net).double()(ob.double())
    p64, v64 = p64.numpy(), v64.numpy()[:, 0]
    x = tower_fp64(net, ob.numpy())
    bias = net.fc1.bias.detach().numpy()
    p, v, lg = head_fp64(x, head_weights(net, "exact"), bias, A)
    assert np.abs(p - p64).max() < 1e-12 and np.abs(v - v64).max() < 1e-12
    # channels past the net's filters (the device's tower output is padded) are ignored
    xp = np.concatenate([x, np.full(x.shape[:2] + (5,), 7.0)], axis=2)
    assert np.array_equal(head_fp64(xp, head_weights(net, "exact"), bias, A)[2], lg)
    # the rounded weights: an f32x pair keeps a weight to 2^-22 of its magnitude (+ 2^-35: the lo half's subnormal spacing / 2048),
    # the hi half alone to 2^-11 (+ 2^-25: fp16's subnormal spacing), so a logit moves by at most that share of sum |x| |w|
    w = np.abs(head_weights(net, "exact")).reshape(A + 1, -1)
    ax = np.abs(x).reshape(x.shape[0], -1)
    for mode, rel, sub in (("tuned", 2.0 ** -22, 2.0 ** -35), ("wide", 2.0 ** -22, 2.0 ** -35), ("f16", 2.0 ** -11, 2.0 ** -25)):
        lr = head_fp64(x, head_weights(net, mode), bias, A)[2]
        bound = ax @ (rel * w + sub).T
        assert (np.abs(lr - lg) <= bound + 1e-12).all(), mode
        assert np.abs(lr - lg).max() > 0, mode
    assert np.array_equal(head_weights(net, "tuned"), head_weights(net, "wide"))


@pytest.mark.parametrize("key", KEYS)
def test_torch_fp32_is_a_usable_end_to_end_yardstick(key):
    """head_cases.yardstick_report: the end-to-end bar of test_head_kernels_gpu measures fp32's precision, not an accident of
    cancellation on one or two boards."""
    for n, bar, pred in hc.yardstick_report(key):
        print("%s n=%d: bar %.3g, predicted fp32 error %.3g" % (key, n, bar, pred))
        if n < 8:
            assert 8.0 * pred <= 2e-6, (n, pred)
        else:
            assert bar >= 2.0 * pred, (n, bar, pred)
