"""What one pnp_drop_loop call may carry over from an earlier call on the same engine: nothing.  Iterations >= 1 of a drop
loop reuse the token embeddings and the text prefix of iteration 0 of the SAME call (csrc/model.hip: pnp_drop_loop_layer);
these tests pin that the reuse never reaches across calls -- not when the caller refills its buffers in place (same pointers,
other contents), and not when other entry points of the engine ran in between.

Geometry and weights of tests/golden/droploop_small.npz (3 images of 128^2, 64 patches, drop_iter 4, head 9): the smallest
case in which iterations >= 1 take the reuse path."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pnp_ovss import config as C, synth            # noqa: E402

pytestmark = pytest.mark.gpu

HEAD, DROP_ITER = 9, 4
SEED_B = 11                                        # images B: any seed other than the golden's (6)


@pytest.fixture(scope="module")
def golden():
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", "droploop_small.npz"), allow_pickle=False)
    assert int(g["image_seed"]) == 6 and int(g["image_seed"]) != SEED_B
    return g


@pytest.fixture(scope="module", params=["f32", "bf16", "bf16x3"])
def case(request, golden):
    """One engine per mode, shared by the two tests, with images A / B and the golden / rolled captions on the host."""
    from pnp_ovss.hip import Engine
    g = golden
    cfg = C.ModelCfg(**json.loads(str(g["cfg"])))
    e = Engine(cfg, max_batch=4, max_text_len=32, stash_layer=7, mode=request.param)
    e.load_state_dict(synth.synth_state_dict(cfg, int(g["weight_seed"])))
    _, imgs_a = synth.synth_images(3, cfg.img_size, seed=int(g["image_seed"]))
    _, imgs_b = synth.synth_images(3, cfg.img_size, seed=SEED_B)
    assert not np.array_equal(imgs_a, imgs_b)
    ids_a, mask_a = g["input_ids"], g["attention_mask"]
    ids_b, mask_b = np.roll(ids_a, 1, axis=0), np.roll(mask_a, 1, axis=0)
    assert not np.array_equal(ids_a, ids_b)
    L = int(mask_a.sum(1).max())
    yield dict(e=e, L=L, imgs_a=torch.from_numpy(imgs_a), imgs_b=torch.from_numpy(imgs_b),
               ids_a=torch.from_numpy(ids_a), mask_a=torch.from_numpy(mask_a),
               ids_b=torch.from_numpy(np.ascontiguousarray(ids_b)), mask_b=torch.from_numpy(np.ascontiguousarray(mask_b)))
    e.close()


def _manual_loop(e, d_img, ids, mask, L, like):
    """The drop loop from the operator-level calls, which compute everything from the images and captions every time."""
    g0, agg, picks, _ = like
    B, PP = d_img.shape[0], e.grid * e.grid
    dropped = torch.zeros(B, PP, dtype=torch.uint8, device="cuda")
    g0m, aggm, picksm = torch.empty_like(g0), torch.empty_like(agg), torch.full_like(picks, -1)
    for it in range(DROP_ITER):
        gc, lg = e.compute_gradcam(d_img, ids, mask, L, HEAD, dropped=dropped)
        e.drop_step(gc, g0m, aggm, dropped, picksm, it)
    torch.cuda.synchronize()
    return g0m, aggm, picksm, lg


def test_drop_loop_after_in_place_refill(case):
    """drop_loop on images / captions A, then B copied into the SAME device tensors, then drop_loop again: the second call's
    gradcam_0, aggregate, picks and logits are bit-identical to a hand-written loop of compute_gradcam(dropped=) + drop_step
    on B.  (Iteration 0 of every call computes the embeddings and the text prefix; only iterations >= 1 of that call reuse.)"""
    e, L = case["e"], case["L"]
    d_img, ids, mask = case["imgs_a"].cuda(), case["ids_a"].cuda(), case["mask_a"].cuda()
    first = e.drop_loop(d_img, ids, mask, L, HEAD, DROP_ITER)
    torch.cuda.synchronize()
    ptrs = (d_img.data_ptr(), ids.data_ptr(), mask.data_ptr())
    d_img.copy_(case["imgs_b"])
    ids.copy_(case["ids_b"])
    mask.copy_(case["mask_b"])
    assert ptrs == (d_img.data_ptr(), ids.data_ptr(), mask.data_ptr())
    g0, agg, picks, logits = e.drop_loop(d_img, ids, mask, L, HEAD, DROP_ITER)
    torch.cuda.synchronize()
    assert not torch.equal(g0, first[0])                                   # B is another batch
    g0m, aggm, picksm, lg = _manual_loop(e, d_img, ids, mask, L, (g0, agg, picks, logits))
    assert torch.equal(picks, picksm)
    assert torch.equal(g0, g0m) and torch.equal(agg, aggm) and torch.equal(logits, lg)


def test_drop_loop_after_other_calls(case):
    """drop_loop on A, then vit_forward on B and text_forward_text on the rolled captions (both overwrite activations the
    loop's reuse reads), then drop_loop on A with the same tensors: the second result equals the first bit for bit."""
    e, L = case["e"], case["L"]
    d_img, ids, mask = case["imgs_a"].cuda(), case["ids_a"].cuda(), case["mask_a"].cuda()
    first = e.drop_loop(d_img, ids, mask, L, HEAD, DROP_ITER)
    torch.cuda.synchronize()
    e.vit_forward(case["imgs_b"].cuda())
    e.text_forward_text(case["ids_b"].cuda(), case["mask_b"].cuda(), L)
    torch.cuda.synchronize()
    second = e.drop_loop(d_img, ids, mask, L, HEAD, DROP_ITER)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
