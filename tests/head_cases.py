"""The nets and batch sizes of the head tests (test_head_kernels_gpu.py on the GPU, test_head_cases_host.py without one): two-block
drifted nets (net_cases.drifted_net) whose fc1 net_cases.trained_head has rewritten, at the action counts where the control flow of
the head kernels changes."""
import copy
import functools

import numpy as np
import torch

from net_cases import boards, drifted_net, head_fp64, head_weights, max_activation_fp64, tower_fp64, trained_head

X3C_FUSED = "az_tower_x3c_kernel (fc1 + softmax + tanh in the same launch)"
HEAD_SMALL = {"f32x": " + az_head_kernel<X3>", "f16": " + az_head_kernel"}
HEAD_GEMM = {"f32x": " + az_head_gemm_kernel<X3> + az_head_softmax_kernel<X3>", "f16": " + az_head_gemm_kernel + az_head_softmax_kernel"}

# key -> (state shape, actions, filters, wide=, seed, batch sizes, also at f16)
# Tuned path (50 filters).  n_ot = ceil((A + 1) / 16) output tiles; az_head_kernel takes n_ot <= 8, the GEMM head the rest.
NETS = {
    "c4_a7": ([3, 6, 7], 7, 50, None, 41, (1, 2, 257, 513, 529), True),       # fused head; az_head_kernel<X3>'s single-tile chain above 512
    "c4_a15": ([3, 6, 7], 15, 50, None, 42, (2, 257), False),                 # one full tile, fused
    "c4_a16": ([3, 6, 7], 16, 50, None, 43, (1, 15, 16, 17, 33), False),      # the value logit alone in tile 2: az_head_kernel's general loop
    "c4_a127": ([3, 6, 7], 127, 50, None, 44, (1, 15, 16, 17, 33), True),     # n_ot == OTG
    "c4_a128": ([3, 6, 7], 128, 50, None, 45, (1, 16, 17, 33, 127, 128, 129), True),  # n_ot == 9: groups of 5 and 4; stride 52, K tail of 24 halves
    "bt6_a432": ([3, 6, 6], 432, 50, None, 46, (1, 17, 33, 127, 129, 1025), True),    # 28 tiles = 4 x 7; 59 k-steps: halves of 30 and 29
    "bt8_a768": ([3, 8, 8], 768, 50, None, 47, (1, 17, 129, 1025), True),     # 49 tiles; HEAD_SM_MAX full, the value read at index 768
    "b5_a300": ([3, 5, 5], 300, 50, None, 48, (1, 33, 129), False),           # odd HW: the GEMM head at stride 64
    # Wide path (az_net_create_wide)
    "w7x9_a255": ([3, 7, 9], 255, 64, None, 49, (1, 33, 129), False),         # 16 tiles: two full groups, NO == 4 only
    "w7x9_a256": ([3, 7, 9], 256, 64, None, 50, (1, 33, 129), True),          # 17 tiles: groups of 6, 6, 5
    # short K: fpad = 32, so fc1 has H*W k-steps.  1x1 is the smallest board az_net_create_wide's validation (rows, cols >= 1) and
    # az_conv_wide_kernel (every tap but the centre masked off the board) take: ONE k-step, halves of 1 and 0 k-steps.  3x1: three
    # k-steps, halves of 2 and 1.  Together: every nk < HG_RING - 1 of the prologue and every count of the loaders' waits.
    "w1x1_a128": ([3, 1, 1], 128, 32, True, 51, (1, 17, 129), False),
    "w3x1_a128": ([3, 3, 1], 128, 24, True, 52, (1, 17, 129), False),
    "wc4_a16": ([3, 6, 7], 16, 50, True, 43, (1, 17, 33), False),             # the wide tower in front of az_head_kernel (c4_a16's net)
}
N_E2E = 64      # the end-to-end check against the float64 Net runs at n <= 64
# trained_head's gate per net, set once from the float64 forward so that the widest policy of the case spans 50 to 100 logits
GATE = {"c4_a7": 1.6, "c4_a15": 1.2, "c4_a16": 2.0, "c4_a127": 2.5, "c4_a128": 1.8, "bt6_a432": 2.2, "bt8_a768": 1.1, "b5_a300": 1.25,
        "w7x9_a255": 1.9, "w7x9_a256": 2.3, "w1x1_a128": 1.6, "w3x1_a128": 0.85, "wc4_a16": 2.0}
HEAD_SEED = {k: v[4] + 100 for k, v in NETS.items()}
HEAD_SEED.update({"c4_a7": 22141, "c4_a127": 20144, "c4_a16": 1143, "wc4_a16": 1143, "bt6_a432": 24146, "bt8_a768": 1147, "w7x9_a256": 1150, "w1x1_a128": 5151})  # found by search on the CPU: the first seed + 1000 j whose float64 forward has trained_head's shares and a usable yardstick (yardstick_report)


@functools.lru_cache(maxsize=None)
def net(key):
    shape, A, F, _, seed = NETS[key][:5]
    return trained_head(drifted_net(shape, A, 2, F, seed), HEAD_SEED[key], gate=GATE[key])


@functools.lru_cache(maxsize=None)
def obs(key):
    """The boards of a case: its largest batch (at least N_E2E); a run of n boards takes the first n."""
    return boards(NETS[key][0], max(max(NETS[key][5]), N_E2E), seed=NETS[key][4])


def mode(key, precision):
    """net_cases.head_weights' mode of the case's device path."""
    if precision == "f16":
        return "f16"
    return "wide" if (NETS[key][3] or NETS[key][2] > 56) else "tuned"


def head_properties(key):
    """What trained_head promises, measured on the float64 forward of the case's net over the case's boards."""
    nt, ob, A = net(key), obs(key), NETS[key][1]
    p, v, lg = head_fp64(tower_fp64(nt, ob.numpy()), head_weights(nt, "exact"), nt.fc1.bias.detach().numpy(), A)
    span = lg[:, :A].max(1) - lg[:, :A].min(1)
    ent = -(p * np.log(np.maximum(p, 1e-300))).sum(1) / np.log(A)
    w, b = np.abs(nt.fc1.weight.detach().numpy()), nt.fc1.bias.detach().numpy()
    return {"span_max": float(span.max()), "wide_span": float((span > 30).mean()), "peaked": float((p.max(1) > 0.99).mean()),
            "uniform": float((ent > 0.8).mean()), "min_prior": float(p.min()), "v_sat": float((np.abs(v) > 0.999).mean()),
            "v_lin": float((np.abs(v) < 0.5).mean()), "w_sub": float((w < 6.1e-5).mean()), "w_sub_lo": float((w < 3e-8).mean()),
            "w_zero": float((w == 0).mean()), "bias_min": float(np.abs(b).min()), "bias_max": float(np.abs(b).max()),
            "bias_distinct": len(set(b.tolist())) == len(b), "logit_max": float(np.abs(lg).max()),
            "top": max_activation_fp64(nt, ob[:N_E2E]), "p": p, "v": v, "logits": lg}


@functools.lru_cache(maxsize=None)
def e2e_reference(key):
    """For the first N_E2E boards of the case: (priors, values) of the float64 Net, torch float32's per-board error against them
    (priors and value), the float64 tower output [B][H*W][F] and torch float32's tower error |t32 - t64| as [B][H*W * F]."""
    nt, ob = net(key), obs(key)[:N_E2E]
    with torch.no_grad():
        p64, v64 = copy.deepcopy(nt).double()(ob.double())
        p32, v32 = nt(ob)
        x = ob
        for blk in nt.blocks():
            x = blk(x)
    p64, v64 = p64.numpy(), v64.numpy()[:, 0]
    t64 = tower_fp64(nt, ob.numpy())
    t32 = np.abs(x.numpy().reshape(x.shape[0], x.shape[1], -1).transpose(0, 2, 1) - t64).reshape(x.shape[0], -1)
    return p64, v64, np.maximum(np.abs(p32.numpy() - p64).max(1), np.abs(v32.numpy()[:, 0] - v64)), t64, t32


def yardstick_report(key):
    """Is torch-fp32's own error a usable yardstick of the end-to-end check at every n <= N_E2E of the case?  The check allows
    4 x that error (at least 2e-6) over the first n boards.  With a head of gain 30 to 80 the output error of ANY fp32-grade forward
    is its tower error seen through the head's Jacobian J = d(priors, value) / d(tower), and on a single board the realised error
    J . dx of one forward can cancel to a small fraction of what its tower error amounts to - the bar then measures that accident, not
    fp32's precision.  Per board b, from the CPU alone: pred_b = rms(torch-fp32's tower error on b) x the largest row norm of J_b (the
    standard deviation of the worst output's error were the tower error unstructured).  Returns [(n, bar, pred)] with bar = max(4 x
    torch-fp32's error over the first n boards, 2e-6) and pred = max of pred_b over them.  test_head_cases_host asserts, for n >= 8
    (the largest of many boards' errors is a stable figure), bar >= 2 x pred: torch's realised error is at least half its own
    prediction; and for n < 8, where one or two boards' realised error is an accident either way (it also differs between machines
    with the thread count of torch's convolutions), 8 x pred <= 2e-6: a forward at the project's limit of 4 x torch stays under the
    bar's floor at two standard deviations, whatever torch's error on those boards happens to be."""
    nt, A = net(key), NETS[key][1]
    p64, v64, e32, t64, t32 = e2e_reference(key)
    w = head_weights(nt, "exact").reshape(A + 1, -1)
    wp, n2 = w[:A], (w ** 2).sum(1)
    pred = np.zeros(len(p64))
    for b, p in enumerate(p64):
        m = p @ wp                                                       # row o of J: p_o (w_o - m)
        rows = p * np.sqrt(np.maximum(n2[:A] - 2.0 * (wp @ m) + m @ m, 0.0))
        pred[b] = np.sqrt((t32[b] ** 2).mean()) * max(rows.max(), (1.0 - v64[b] ** 2) * np.sqrt(n2[A]))
    return [(n, max(4.0 * float(e32[:n].max()), 2e-6), float(pred[:n].max())) for n in NETS[key][5] if n <= N_E2E]
