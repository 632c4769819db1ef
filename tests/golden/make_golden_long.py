#!/usr/bin/env python3
"""Golden vectors for horizons above 128 positions, made by the REAL reference (same import harness and helpers as
make_golden.py, which this module imports).  Forward cases: one U-Net forward and its fp64 run with the reference's
own modules, and a conditioned sampling loop of the net's schedule length with injected noise.  Gradient cases: the
loss of diffusion.py:253-290 on injected draws, loss.backward(), every parameter gradient (sampled as grads_*) and
d loss / d x_t.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_long.py [--cases NAME[,NAME...]]

Inputs come from cases.horizon_inputs / cases.loop_condition / cases_long.long_train_inputs under the case names of
cases_long.py (regenerable).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests.golden import cases                                        # noqa: E402
from tests.golden.cases_long import LONG_CASES, LONG_GRAD_CASES, long_train_inputs  # noqa: E402
from tests.golden import make_golden as mg                           # noqa: E402  (imports the reference)


def gen_long(only=()):
    for case, net, Hz, B, t in LONG_CASES:
        if only and case not in only:
            continue
        print(f"  long horizon {case} ...")
        od, ad, td, dim, mults = cases.net_dims(net)
        T = cases.NETS[net][4]
        unet = mg.ref_unet.TemporalUnet(td, dim=dim, dim_mults=tuple(mults)).eval()
        mg.load_into(unet, cases.net_weights(net))
        diff = mg.GaussianDiffusion(unet, Hz, od, ad, n_timesteps=T, beta_schedule="cosine").eval()
        x, noise = cases.horizon_inputs(case, net, Hz, B, T)
        tt = torch.full((B,), t, dtype=torch.long)
        with torch.no_grad():
            eps = unet(torch.from_numpy(x), tt)
            u64 = mg.ref_unet.TemporalUnet(td, dim=dim, dim_mults=tuple(mults)).eval()
            mg.load_into(u64, cases.net_weights(net))
            u64 = u64.double()
            pos = u64.time_mlp[0]
            orig = pos.forward
            pos.forward = lambda tt_, orig=orig: orig(tt_).double()
            eps64 = u64(torch.from_numpy(x).double(), tt)
        pol = mg.ref_pol.GuidedPolicy(diff, normalizer=None)
        cond = {0: torch.from_numpy(cases.loop_condition(case, net))}
        with mg.injected_noise(noise):
            xf = pol.sample_loop(batch_size=B, conditions=cond)
        mg.save(case, eps=eps.numpy(), eps_fp64=eps64.numpy(), x_final=xf.numpy())


def gen_long_grads(only=()):
    for case, net, Hz, T, B, loss_type, pred_eps in LONG_GRAD_CASES:
        if only and case not in only:
            continue
        print(f"  long horizon grads {case} ...", flush=True)
        od, ad, td, dim, mults = cases.net_dims(net)
        unet = mg.ref_unet.TemporalUnet(td, dim=dim, dim_mults=tuple(mults))
        mg.load_into(unet, cases.net_weights(net))
        diff = mg.GaussianDiffusion(unet, Hz, od, ad, n_timesteps=T, beta_schedule="cosine", loss_type=loss_type,
                                    predict_epsilon=pred_eps).train()
        x0, t, noise = long_train_inputs(case, net, Hz, T, B)
        x0t, tt, nz = torch.from_numpy(x0), torch.from_numpy(t), torch.from_numpy(noise)
        x_t = diff.q_sample(x0t, tt, nz).detach().requires_grad_(True)
        out = diff.model(x_t, tt)
        loss = diff.loss_fn(out, nz if pred_eps else x0t).mean()
        diff.zero_grad()
        loss.backward()
        arrays = {"loss": np.float64(loss.item()), "dx": x_t.grad.numpy()}
        for k, p in diff.model.named_parameters():
            g = p.grad.numpy().reshape(-1)
            idx = cases.grad_sample_index(g.size)
            arrays["g." + k] = g[idx]
            arrays["sum." + k] = np.float64(g.astype(np.float64).sum())
            arrays["sq." + k] = np.float64((g.astype(np.float64) ** 2).sum())
            arrays["max." + k] = np.float64(np.abs(g).max())
        mg.save(case, **arrays)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="", help="comma-separated fixture names")
    args = ap.parse_args()
    torch.manual_seed(0)
    only = tuple(c for c in args.cases.split(",") if c)
    gen_long(only)
    gen_long_grads(only)
