"""Text towers alone at the bench shape (bs = 256, T = 40, bf16, dropout on):
forward + backward per step with HIP events after warm-up, for
  * the TinyBERT tower (CLS-only last layer, as the training step runs it),
  * the DistilBERT tower (CLS-only last layer, and the full last layer),
  * transformers.DistilBertModel under torch.autocast(bf16) on the same GPU in the
    same process (the stock PyTorch-ROCm module the DistilBERT tower replaces; it
    computes the full last layer, so the full-path time is the like-for-like one),
and the per-family kernel time (ktimer) of one step of each HIP tower, to size what
the text stream costs the step when it shares the CUs with the image tower.
  python tools/text_tower_bench.py [--batch 256] [--seq 40] [--iters 20] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]
import torch  # noqa: E402


def timed(step, iters, reps=5):
    """median over `reps` event-timed windows of `iters` steps, after warm-up"""
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return round(statistics.median(ms), 3), [round(v, 3) for v in ms]


def families(step):
    from vlp_amd import ktimer
    ktimer.enable(None)
    step()
    torch.cuda.synchronize()
    fam = {k: round(v[0], 4) for k, v in sorted(ktimer.totals().items(), key=lambda kv: -kv[1][0])}
    ktimer.disable()
    return fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=40)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vlp_amd.distilbert import DistilBertConfig, DistilBertTower
    from vlp_amd.tinybert import TinyBertConfig, TinyBertTower
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, 30000, (a.batch, a.seq), generator=g).to(dev)
    mask = torch.ones(a.batch, a.seq, dtype=torch.long, device=dev)
    mask[:, a.seq * 3 // 4:] = 0
    tt = torch.zeros_like(ids)
    res = {"shape": f"bs={a.batch} T={a.seq} bf16 dropout 0.1", "device": torch.cuda.get_device_name(0)}

    def hip_steps(t):
        dcls = torch.randn(a.batch, t.cfg.hidden, device=dev) * 1e-3

        def step(cls_only=True):
            h, sv = t.run_forward(ids, mask, tt, True, cls_only=cls_only)
            t.run_backward(sv, dcls)
        return step

    tiny = hip_steps(TinyBertTower(TinyBertConfig(0.1, 0.1), compute_dtype="bf16", device=dev).train())
    res["tinybert_hip_ms"], res["tinybert_hip_windows"] = timed(tiny, a.iters)
    res["tinybert_families_ms"] = families(tiny)
    dist = hip_steps(DistilBertTower(DistilBertConfig(0.1, 0.1), compute_dtype="bf16", device=dev).train())
    res["distilbert_hip_ms"], res["distilbert_hip_windows"] = timed(dist, a.iters)
    res["distilbert_hip_full_ms"], res["distilbert_hip_full_windows"] = timed(lambda: dist(False), a.iters)
    res["distilbert_families_ms"] = families(dist)

    from transformers import DistilBertConfig as HFConfig, DistilBertModel
    hf = DistilBertModel(HFConfig()).to(dev).train()
    dcls = torch.randn(a.batch, 768, device=dev) * 1e-3

    def hf_step():
        hf.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = hf(input_ids=ids, attention_mask=mask).last_hidden_state
        (h[:, 0, :].float() * dcls).sum().backward()

    res["distilbert_torch_autocast_ms"], res["distilbert_torch_autocast_windows"] = timed(hf_step, a.iters)
    res["attn_implementation"] = hf.config._attn_implementation
    res["torch_over_hip_full"] = round(res["distilbert_torch_autocast_ms"] / res["distilbert_hip_full_ms"], 3)
    res["torch_over_hip_cls_only"] = round(res["distilbert_torch_autocast_ms"] / res["distilbert_hip_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
