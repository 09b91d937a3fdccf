"""Worker of tests/test_gpu_head_masked.py::test_world2_gloo_masked (not collected
by pytest): one rank of a world-size-2 run of the contrastive head with the
duplicate-caption mask.

Launched by torch.distributed.run with the gloo backend, both ranks on the one
GPU of the test box (vlp_amd.dist stages device tensors through host memory
under gloo).  Each rank takes its B rows of the 2B-row embeddings the test
draws and its B caption strings, and runs what ClipStepFn runs between the
projections and the backward: caption_hash64 of its strings, global_batch_loss
(all-gather of embeddings and caption keys, vlp_clip_loss_fused_masked at
offset rank * B, all-reduce of the loss terms) and the reduce-scatter of the
gathered-embedding gradients.  It writes the loss, its gradient rows and the
gathered ids to <outdir>/r<rank>.pt.
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    outdir, B, E, captions = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4].split(",")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from tests.test_gpu_head_masked import embeddings
    from vlp_amd import dist as vdist
    from vlp_amd.clip_model import caption_hash64, global_batch_loss

    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    ie, te = embeddings(world * B, E, 21)
    sl = slice(rank * B, (rank + 1) * B)
    ls = torch.tensor([math.log(1 / 0.07)], dtype=torch.float32, device=dev)
    out, g_img_all, g_txt_all, small, gathered = global_batch_loss(
        ie[sl].to(dev).contiguous(), te[sl].to(dev).contiguous(), ls, caption_hash64(captions[sl]))
    g_img = vdist.reduce_scatter_rows(g_img_all)
    g_txt = vdist.reduce_scatter_rows(g_txt_all)
    torch.cuda.synchronize()
    torch.save({"loss": out[0].item(), "g_img": g_img.cpu(), "g_txt": g_txt.cpu(), "cid_all": gathered[4].cpu()},
               os.path.join(outdir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
