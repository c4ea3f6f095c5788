"""MASt3R on the device, from images to the reference's `inference()` output: the trunk (mast3r_trunk.py) and both heads
(mast3r_heads.py) built from ONE read of the checkpoint, and the hand-over to the global aligner — the step of init_geo.py:45-50
between `load_images` and `global_aligner(...)`.  Recalled block definitions throughout (see the two modules): parity with a
trained model is unpinned."""
from __future__ import annotations

import torch

from .global_align import AlignProblem
from .mast3r_heads import HeadsConfig, Mast3rHeads, load_checkpoint_model
from .mast3r_trunk import DEFAULT_SCRATCH_BUDGET, Mast3rTrunk, TrunkConfig, complete_edges


class Mast3r:
    def __init__(self, state_dict, trunk_config: TrunkConfig | None = None, heads_config: HeadsConfig | None = None, device=None):
        self.trunk = Mast3rTrunk(state_dict, trunk_config, device=device)
        self.heads = Mast3rHeads(state_dict, heads_config, device=device)

    @classmethod
    def from_checkpoint(cls, path, trunk_config: TrunkConfig | None = None, heads_config: HeadsConfig | None = None, device=None):
        return cls(load_checkpoint_model(path), trunk_config, heads_config, device=device)

    def inference(self, images: torch.Tensor, edges=None, descriptors=False, scratch_budget: int = DEFAULT_SCRATCH_BUDGET) -> dict:
        """images float32 [V,3,H,W] as `load_images` normalises them; edges=None: `make_pairs`' complete symmetrized graph ->
        the dict of dust3r/inference.py:51 for the batch of E edges, on the device:
          view1 / view2: idx (int64 [E], the edge's image i / j), true_shape (int32 [E,2] = (H, W))
          pred1: pts3d [E,H,W,3], conf [E,H,W] (+ desc [E,H,W,D], desc_conf [E,H,W] with descriptors=True)
          pred2: pts3d_in_other_view, conf (+ desc, desc_conf)
          edges: int64 [E,2], in the order of the rows;  loss: None."""
        feat, _, dec1, dec2, e = self.trunk.forward_pairs(images, edges, scratch_budget)
        H, W = int(images.shape[2]), int(images.shape[3])
        p = self.trunk.config.patch
        out1, out2 = self.heads.heads(dec1, dec2, (H // p, W // p), descriptors=descriptors, scratch_budget=scratch_budget)
        out2["pts3d_in_other_view"] = out2.pop("pts3d")   # dust3r/model.py:209: view 2's points in view 1's frame
        shape = torch.tensor([[H, W]], dtype=torch.int32).expand(int(e.shape[0]), 2).contiguous()
        return dict(view1=dict(idx=e[:, 0].clone(), true_shape=shape), view2=dict(idx=e[:, 1].clone(), true_shape=shape.clone()),
                    pred1=out1, pred2=out2, edges=e, loss=None)

    def align_problem(self, images: torch.Tensor, edges=None, scratch_budget: int = DEFAULT_SCRATCH_BUDGET, **switches) -> AlignProblem:
        """`inference` handed to the aligner as the reference's PointCloudOptimizer takes it (pred_i = pred1.pts3d, pred_j =
        pred2.pts3d_in_other_view, the raw confidences); switches: AlignProblem's keyword arguments"""
        out = self.inference(images, edges, scratch_budget=scratch_budget)
        H, W = int(images.shape[2]), int(images.shape[3])
        return AlignProblem(out["edges"].tolist(), out["pred1"]["pts3d"], out["pred2"]["pts3d_in_other_view"], out["pred1"]["conf"],
                            out["pred2"]["conf"], H, W, **switches)


__all__ = ["Mast3r", "HeadsConfig", "TrunkConfig", "complete_edges"]
