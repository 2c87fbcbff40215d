"""The object-token batches shared by tests/test_obj_static_host.py (CPU) and tests/test_gpu_zz_obj_static.py: a tiny
REVERIE-style configuration and seeded ragged batches whose per-sample step counts and per-panorama object counts differ
while their padded shapes agree (the seeds are pinned by test_batches_with_other_step_and_object_counts_share_a_bucket)."""
import numpy as np

from vln_bevbert_amd import synthetic
from vln_bevbert_amd.config import BevBertConfig

CFG = BevBertConfig.tiny(image_feat_size=768, obj_feat_size=768, obj_prob_size=50, num_l_layers=1, num_x_layers=1,
                         vocab_size=400, pretrain_tasks=("mlm", "mrc", "sap", "og"))
SHAPES_A = ((5, 70), (2, 48), (4, 76))          # (steps, text length) per sample
SHAPES_B = ((3, 66), (6, 50), (2, 75))          # other step counts: the same number of panoramas after padding
SEED_A, SEED_B, SEED_OTHER_WIDTH = 71, 75, 77          # A / B share a bucket; 77 on SHAPES_B has another joint [views | objects] width


def make(seed, task, shapes=SHAPES_A, max_objects=None):
    rng = np.random.default_rng(seed)
    samples = [synthetic.make_sample(rng, i, CFG, T, L, ragged_views=True, max_objects=max_objects)
               for i, (T, L) in enumerate(shapes)]
    return synthetic.collate(samples, CFG, task, rng)
