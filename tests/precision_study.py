#!/usr/bin/env python3
"""Regenerates the precision table of DESIGN.md §2 on the CPU oracle.  (A script, not a test: it lives under tests/
because it imports oracle/, which only tests/, smoke() and bench.py's cpu_baseline leg may do.)

Every nn.Linear of the oracle (trunk + head: the 48 + 4 GEMMs of a forward) -- and, with --attn, the two attention
products -- is replaced by a product whose OPERANDS are rounded the way a candidate MFMA scheme would feed them, with
fp32 accumulation (the CPU's fp32 dot product stands in for the MFMA accumulator):

    fp32            reference
    bf16 / fp16     one pass, both operands rounded to the format
    bf16x3          x = hi + lo (two bf16 terms, 16 significant bits): hi*hi + hi*lo + lo*hi        (3 MFMA passes)
    fp16x2_act      activations hi + lo (two fp16 terms, 22 bits), weights one fp16 term            (2 passes)
    fp16x2_w        weights hi + lo, activations one fp16 term                                      (2 passes)
    bf16x2_act / bf16x2_w   the same with bf16 terms                                                 (2 passes)
    fp16x3          both operands as two fp16 terms, three products                                 (3 passes)

Reported: max |logit error| against the fp32 run (north_star's bound is 1e-3) for the forward schemes, and the
per-tensor relative L2 error of the gradients (median / max over the 215 tensors) for backward schemes (forward kept
fp32-grade = bf16x3, the engine's choice).  `--trajectory N` additionally trains N optimizer steps with each backward
scheme against the fp32 run (dropout 0) and prints the loss drift: the CPU rehearsal of tests/test_gpu_trajectory.py.

`--slices` prints the table behind the per-slice gradient bounds of tests/grad_check.py: the oracle under
`engine_noise_model()` -- every rounding point of the engine's step restated on the oracle side -- against the plain oracle,
the worst of each statistic of grad_check.grad_stats over all gradient tensors and where it occurs, per shape and seed.

    python tests/precision_study.py --layers 12 --batch 8            # the table of DESIGN.md §2 (a few minutes on 8 cores)
    python tests/precision_study.py --slices                         # the table of DESIGN.md §5 (two minutes on 8 cores)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import TASK_CFG, uc2_cfg_dict  # noqa: E402
from oracle import adamw_oracle as A  # noqa: E402
from oracle import uc2_oracle as O  # noqa: E402
from clg_vqa_amd.config import BertConfig  # noqa: E402
from clg_vqa_amd.synthetic import make_batch, seeded_state_dict  # noqa: E402


def _terms(x, fmt, n):
    """x ~= sum of n terms of format fmt (each exactly representable), as fp32 tensors."""
    dt = torch.bfloat16 if fmt == "bf16" else torch.float16
    out, r = [], x
    for _ in range(n):
        t = r.to(dt).to(torch.float32)
        out.append(t)
        r = r - t
    return out


def qmm(a, b, scheme):
    """a [.., M, K] @ b [.., K, N] with operands fed as `scheme` says; a = activations / left, b = weights / right."""
    if scheme == "fp32":
        return a @ b
    if scheme in ("bf16", "fp16"):
        return _terms(a, scheme, 1)[0] @ _terms(b, scheme, 1)[0]
    fmt = scheme[:4]
    if scheme.endswith("x3"):
        ah, al = _terms(a, fmt, 2)
        bh, bl = _terms(b, fmt, 2)
        return al @ bh + ah @ bl + ah @ bh
    if scheme.endswith("x2_act"):
        ah, al = _terms(a, fmt, 2)
        bh = _terms(b, fmt, 1)[0]
        return al @ bh + ah @ bh
    if scheme.endswith("x2_w"):
        ah = _terms(a, fmt, 1)[0]
        bh, bl = _terms(b, fmt, 2)
        return ah @ bl + ah @ bh
    raise ValueError(scheme)


class QLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, fwd, bwd):
        ctx.save_for_backward(x, w)
        ctx.bwd = bwd
        y = qmm(x.reshape(-1, x.shape[-1]), w.t(), fwd).reshape(*x.shape[:-1], w.shape[0])
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
        dx = qmm(dy2, w, ctx.bwd).reshape(x.shape)
        dw = qmm(dy2.t(), x2, ctx.bwd)
        return dx, dw, dy2.sum(0), None, None


class QMatmul(torch.autograd.Function):
    """The two products of the attention core (Q K^T and P V) with a scheme per direction.  With bwd = "bf16" the backward
    products read what the engine's attention backward reads: dctx as bf16 (dP = dctx V^T, dV = P^T dctx), P rounded to bf16
    (dV), dS rounded to bf16 (dQ = dS K, dK = dS^T Q), and the bf16 halves of q, k, v."""

    @staticmethod
    def forward(ctx, a, b, fwd, bwd):
        ctx.save_for_backward(a, b)
        ctx.bwd = bwd
        return qmm(a, b, fwd)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        return qmm(dy, b.transpose(-1, -2), ctx.bwd), qmm(a.transpose(-1, -2), dy, ctx.bwd), None, None


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


class GeluBf16Grad(torch.autograd.Function):
    """erf-GELU whose backward is the engine's: GELU'(x) is stored as bf16 by the forward epilogue and multiplied into the bf16
    result of the dX product behind it; the product is the (bf16) dY operand of the next backward GEMM (rounded there)."""

    @staticmethod
    def forward(ctx, x):
        cdf = 0.5 * (1.0 + torch.erf(x / np.sqrt(2.0)))
        ctx.save_for_backward(_bf16(cdf + x * torch.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)))
        return x * cdf

    @staticmethod
    def backward(ctx, dy):
        return _bf16(dy) * ctx.saved_tensors[0]


class Patched(object):
    """Context: nn.Linear (and optionally torch.matmul of the attention core) run through qmm.  attn= is one scheme for the
    attention products in both directions (through autograd of qmm); attn_fwd= / attn_bwd= give each direction its own
    (QMatmul); gelu_bf16 restates the bf16 GELU' of the trunk's feed-forward backward (the head computes its GELU' in fp32)."""

    def __init__(self, fwd, bwd="fp32", attn=None, attn_fwd=None, attn_bwd=None, gelu_bf16=False):
        assert not (attn and (attn_fwd or attn_bwd))
        self.fwd, self.bwd, self.attn, self.gelu_bf16 = fwd, bwd, attn, gelu_bf16
        self.attn_fwd, self.attn_bwd = attn_fwd, attn_bwd

    def __enter__(self):
        self._lin, self._mm = torch.nn.functional.linear, torch.matmul
        self._gelu, self._head_gelu = O.gelu_erf, O._GeLU.forward
        fwd, bwd = self.fwd, self.bwd
        torch.nn.functional.linear = lambda x, w, b=None: QLinear.apply(x, w, b, fwd, bwd)
        if self.attn:
            attn = self.attn
            torch.matmul = lambda a, b: qmm(a, b, attn)
        elif self.attn_fwd or self.attn_bwd:
            af, ab = self.attn_fwd or "fp32", self.attn_bwd or "fp32"
            torch.matmul = lambda a, b: QMatmul.apply(a, b, af, ab)
        if self.gelu_bf16:
            exact = self._gelu
            O.gelu_erf = GeluBf16Grad.apply
            O._GeLU.forward = lambda self_, x: exact(x)
        return self

    def __exit__(self, *exc):
        torch.nn.functional.linear, torch.matmul = self._lin, self._mm
        O.gelu_erf, O._GeLU.forward = self._gelu, self._head_gelu


def engine_noise_model():
    """The reference-side model of the engine's rounding: forward products -- every Linear and the attention
    core -- as 3-term split bf16; every backward product single-pass bf16, i.e. both operands rounded to bf16 where they are
    fed.  That places the engine's backward rounding points on the oracle side:
      * dctx (the out-projection's dX result) is fed to the attention backward as bf16       -- QMatmul.backward, dy of P V
      * P and dS are rounded to bf16 inside the attention backward                             -- QMatmul.backward, a / dy
      * dqkv leaves the attention backward as bf16, the LayerNorm backward's dpre16 is bf16   -- QLinear.backward, dy
      * GELU' is saved as bf16 and multiplied into the bf16 dX result of FFN2                  -- GeluBf16Grad
    Accumulation is fp32 on both sides.  The bounds of tests/grad_check.py come from this model, never from the engine."""
    return Patched("bf16x3", "bf16", attn_fwd="bf16x3", attn_bwd="bf16", gelu_bf16=True)


def build(layers, vocab, seed, dropout0=False, **width):
    cfg = uc2_cfg_dict(n_layers=layers, vocab=vocab, **width)
    if dropout0:
        cfg.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    config = BertConfig.from_dict(cfg)
    model = O.OracleUC2ForVLTasks(config, TASK_CFG, ["TASK15"], dropout_prob=0.0 if dropout0 else 0.1)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=seed), strict=True)
    return model


def run(model, batch, fwd, bwd, attn=None, grads=True):
    model.eval()
    model.zero_grad()
    with Patched(fwd, bwd, attn):
        loss, _, logits = O.forward_train(model, batch)
        if grads:
            loss.backward()
    g = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None} if grads else None
    return logits.detach(), g


# (name, layers, B, T, V, vocab, width): the shapes of tests/test_gpu_model.py whose noise sets the per-slice bounds
SLICE_CASES = [("L2 B8 T20 V36", 2, 8, 20, 36, 2000, {}), ("L2 B3 T7 V9", 2, 3, 7, 9, 2000, {}),
               ("L2 B2 T20 V100", 2, 2, 20, 100, 2000, {}), ("L2 B1 T6 V4", 2, 1, 6, 4, 2000, {}),
               ("L12 B8 T20 V36", 12, 8, 20, 36, 2000, {}),
               ("c1 (H128, 4 heads) L2 B4 T20 V36", 2, 4, 20, 36, 1000, dict(hidden=128, heads=4, inter=512))]
SLICE_MARGINS = dict(scale=3.0, row=4.0, column=4.0, element=4.0)


def noise_model_grads(model, batch):
    """({name: gradient} of the plain fp32 oracle, the same under engine_noise_model()), eval mode: every parameter plus
    "features.grad" [B, V, 2048] and "spatials.grad" [B, V, 7], the two input gradients the engine returns."""
    model.eval()
    out = []
    for ctx in (Patched("fp32", "fp32"), engine_noise_model()):
        model.zero_grad()
        feats, spat = batch[0].clone().requires_grad_(True), batch[1].clone().requires_grad_(True)
        with ctx:
            loss, _, _ = O.forward_train(model, (feats, spat) + tuple(batch[2:]))
            loss.backward()
        g = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        g["features.grad"], g["spatials.grad"] = feats.grad, spat.grad
        out.append(g)
    return out[0], out[1]


def one_digit(x):
    """x rounded to one significant digit."""
    e = int(np.floor(np.log10(x)))
    return round(x / 10.0 ** e) * 10.0 ** e


def slices(args):
    import grad_check as G
    overall = G.Worst()
    print("noise model (engine_noise_model) vs the plain oracle: worst of each statistic over all gradient tensors, and where")
    print("| shape | seed | tensor | scale | row | column | element |")
    print("|---|---|---|---|---|---|---|")
    for name, layers, B, T, V, vocab, width in SLICE_CASES:
        for seed in range(args.seeds):
            model = build(layers, vocab, 40 + seed, **width)
            batch = make_batch(B, seq_len=T, num_boxes=V, vocab_size=vocab, seed=500 + seed)
            batch[2][0, V - 3:] = 0  # a padded image region, as in the model tests
            gref, g = noise_model_grads(model, batch)
            worst = G.check_grads(g, gref, check=False)
            cells = []
            for k in G.STATS:
                v, n = worst[k]
                st = G.grad_stats(g[n], gref[n])
                at = "[%d]" % st["where"][k][0] if k in st["where"] else ""
                cells.append("%.2e %s%s" % (v, n.replace("bert.", "").replace("encoder.", ""), at))
                if v > overall[k][0]:
                    overall[k] = (v, "%s, seed %d, %s%s" % (name, seed, n, at))
            print("| %s | %d | %s |" % (name, seed, " | ".join(cells)), flush=True)
    print("\n| statistic | worst of the noise model | where | margin | bound (one significant digit) |")
    print("|---|---|---|---|---|")
    for k in G.STATS:
        v, at = overall[k]
        if k in SLICE_MARGINS:
            print("| %s | %.2e | %s | %.0fx | %.0e |" % (k, v, at, SLICE_MARGINS[k], one_digit(v * SLICE_MARGINS[k])))
        else:
            print("| %s | %.2e | %s | - | %.0e (the existing per-tensor bound) |" % (k, v, at, G.GRAD_REL_L2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", action="store_true", help="the per-slice gradient noise table of DESIGN.md section 5")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=2000)
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--trajectory", type=int, default=0)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--traj-layers", type=int, default=2, help="depth of the trajectory rehearsal")
    ap.add_argument("--traj-lr-scale", type=float, default=1.0)
    ap.add_argument("--traj-only", action="store_true", help="skip the single-step tables")
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    if args.slices:
        return slices(args)
    fwd_schemes = ["bf16", "fp16", "bf16x2_act", "bf16x2_w", "fp16x2_act", "fp16x2_w", "bf16x3", "fp16x3"]
    if args.traj_only:
        return trajectory(args)
    print("forward schemes: %d layers, batch %d, %d seed(s); max |logit error| vs fp32 (logit std in brackets)" % (
        args.layers, args.batch, args.seeds))
    res = {s: [] for s in fwd_schemes + ["bf16x3+attn_bf16x3"]}
    stds = []
    for seed in range(args.seeds):
        model = build(args.layers, args.vocab, 40 + seed)
        batch = make_batch(args.batch, vocab_size=args.vocab, seed=500 + seed)
        ref, _ = run(model, batch, "fp32", "fp32", grads=False)
        stds.append(ref.std().item())
        for s in fwd_schemes:
            lg, _ = run(model, batch, s, "fp32", grads=False)
            res[s].append((lg - ref).abs().max().item())
        lg, _ = run(model, batch, "bf16x3", "fp32", attn="bf16x3", grads=False)
        res["bf16x3+attn_bf16x3"].append((lg - ref).abs().max().item())
    passes = {"bf16": 1, "fp16": 1, "bf16x3": 3, "fp16x3": 3, "bf16x3+attn_bf16x3": 3}
    print("| scheme | MFMA passes | max abs logit error (worst seed) | fits 1e-3 |")
    print("|---|---|---|---|")
    for s, v in res.items():
        print("| %s | %d | %.2e (logit std %.2f) | %s |" % (s, passes.get(s, 2), max(v), np.mean(stds),
                                                            "yes (%.0fx margin)" % (1e-3 / max(v)) if max(v) < 1e-3 else "NO"))
    # backward schemes (forward fixed at the engine's bf16x3)
    print("\nbackward schemes (forward bf16x3): per-tensor gradient rel-L2 error vs the fp32 run, median / max")
    model = build(args.layers, args.vocab, 40)
    batch = make_batch(args.batch, vocab_size=args.vocab, seed=500)
    _, gref = run(model, batch, "fp32", "fp32")
    print("| backward operands | passes | median | max | worst tensor |")
    print("|---|---|---|---|---|")
    for s in ("bf16", "fp16", "bf16x2_act", "bf16x3"):
        _, g = run(model, batch, "bf16x3", s, attn=("bf16" if s == "bf16" else None))
        rel = {n: ((g[n] - gref[n]).double().norm() / gref[n].double().norm().clamp_min(1e-30)).item()
               for n in gref if not n.endswith("attention_self.key.bias")}
        worst = max(rel, key=rel.get)
        print("| %s%s | %d | %.2e | %.2e | %s |" % (s, " (+ bf16 attention core)" if s == "bf16" else "", passes.get(s, 2),
                                                    float(np.median(list(rel.values()))), rel[worst], worst))
    if args.trajectory:
        trajectory(args)


def trajectory(args):
    if True:
        print("\ntrajectory: %d optimizer steps (dropout 0, lr %.1e, wd 1e-4, clip 1.0, warm-up 2 of 20), %d layers, batch 8"
              % (args.trajectory, 4e-5 * args.traj_lr_scale, args.traj_layers))
        hp = dict(base_lr=4e-5 * args.traj_lr_scale, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-6, correct_bias=True, warmup_steps=2,
                  t_total=20, max_grad_norm=1.0)
        batches = [make_batch(8, vocab_size=args.vocab, seed=900 + i) for i in range(4)]
        runs = {}
        # "bf16x3 fwd / fp32 bwd" differs from fp32 by ~2e-5 on the logits only: it shows how fast ANY perturbation of that size
        # grows over the steps (the chaos floor of this bs-8 run), against which the bf16 / fp16 backward schemes are read
        for name, (f, b) in {"fp32": ("fp32", "fp32"), "bf16x3 fwd / bf16 bwd": ("bf16x3", "bf16"),
                             "bf16x3 fwd / fp32 bwd": ("bf16x3", "fp32"), "bf16x3 fwd / fp16 bwd": ("bf16x3", "fp16"),
                             "bf16x3 fwd / bf16x2_act bwd": ("bf16x3", "bf16x2_act")}.items():
            m = build(args.traj_layers, args.vocab, 77, dropout0=True)
            m.train()
            opt = A.ReferenceAdamW(m.named_parameters(), **hp)
            losses = []
            for s in range(args.trajectory):
                with Patched(f, b):
                    loss, _, _ = O.forward_train(m, batches[s % 4])
                    loss.backward()
                opt.step()
                losses.append(float(loss))
            runs[name] = (losses, {n: p.detach().clone() for n, p in m.named_parameters()})
        base = runs["fp32"][0]
        for name, (losses, _) in runs.items():
            print("%-28s rel drift vs fp32 per step: %s   max %.2e" % (
                name, " ".join("%.1e" % (abs(a - b) / abs(b)) for a, b in zip(losses, base)),
                max(abs(a - b) / abs(b) for a, b in zip(losses, base))), flush=True)


if __name__ == "__main__":
    main()
