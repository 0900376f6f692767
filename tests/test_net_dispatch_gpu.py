"""Which kernels a PV-net forward launches (csrc/az_net.hip: plan_forward), pinned: az_net_kernel_label and
az_net_issued_mfma_per_board for every net shape of test_fused_net, a 64-filter net (the wide path) and a 50-filter net the tuned
path refuses at f32x, at both precisions and every batch size of BATCHES, must equal tests/golden/net_dispatch.json exactly.
The record was made from the library before plan_forward existed (tools/make_net_dispatch_fixture.py).  bench.py --full
computes its roofline from the MFMA count and names the kernel from the label; profiling finds rocprof rows by the label."""
import functools
import json
import os

import pytest
import torch

from conftest import GOLDEN
from alphazero_openspiel_amd import fusednet
from alphazero_openspiel_amd.network import Net
from test_fused_net import _nets

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, 128, 129, 256, 257, 300, 512, 513, 700, 1024, 1025, 1280, 1500, 2048, 4096)
MAX_BOARDS = 4096
FIXTURE = os.path.join(GOLDEN, "net_dispatch.json")


@functools.lru_cache(maxsize=1)
def dispatch_nets():
    """tag -> net; only the shape matters, except for the refused net's one large weight."""
    nets = {tag: net for tag, (_, net) in _nets().items()}
    torch.manual_seed(4)
    nets["c4_64f_2block"] = Net([3, 6, 7], 7, n_blocks=2, n_filters=64).eval()
    refused = Net([3, 6, 7], 7, n_blocks=2, n_filters=50).eval()
    with torch.no_grad():
        refused.resblock2.conv1.weight[3, 7, 1, 1] = 100.0  # the tuned path keeps f32x weights x 2048 in fp16: refused there
    nets["c4_50f_w100"] = refused
    return nets


def record(net, precision):
    """The label at n_boards = 0 through the C ABI (the reserved maximum), then label and MFMA count at every batch size."""
    fn = fusednet.FusedNet(net, "cuda:0", max_boards=MAX_BOARDS, precision=precision)
    try:
        return {"label_0": fn.lib.az_net_kernel_label(fn._h, 0).decode(),
                "labels": [fn.kernel_label(n) for n in BATCHES],
                "mfma": [fn.issued_mfma_per_board(n) for n in BATCHES]}
    finally:
        fn.close()


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _kind(label):
    """plan_forward's tower kind of a label."""
    if label.startswith("az_tower_x3c_kernel (fc1 + softmax + tanh"):
        return "X3C_FUSED_HEAD"
    return {"az_tower_kernel": "F16", "az_tower_f16c_kernel": "F16C", "az_tower_x3_kernel": "X3", "az_tower_x3b_kernel": "X3B",
            "az_tower_x3c_kernel": "X3C", "az_tower_x3d_kernel": "X3D", "az_wide_input_kernel": "WIDE"}[label.split(" ")[0]]


def test_the_record_covers_every_tower_kind():
    rec = _fixture()
    assert rec["batches"] == list(BATCHES) and rec["max_boards"] == MAX_BOARDS
    assert sorted(rec["nets"]) == sorted(dispatch_nets())
    kinds = {_kind(lab) for per in rec["nets"].values() for r in per.values() for lab in r["labels"] + [r["label_0"]]}
    assert kinds == {"F16", "F16C", "X3", "X3B", "X3C", "X3C_FUSED_HEAD", "X3D", "WIDE"}


@pytest.mark.parametrize("precision", fusednet.PRECISIONS)
def test_kernel_label_and_mfma_count_match_the_record(precision):
    rec = _fixture()["nets"]
    for tag, net in dispatch_nets().items():
        got = record(net, precision)
        want = rec[tag][precision]
        assert got["label_0"] == want["label_0"], (tag, precision)
        for n, gl, wl, gm, wm in zip(BATCHES, got["labels"], want["labels"], got["mfma"], want["mfma"]):
            assert gl == wl, (tag, precision, n)
            assert gm == wm, (tag, precision, n)
