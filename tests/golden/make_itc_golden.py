#!/usr/bin/env python
"""Golden vectors of the ITC head and of extract_features, produced by RUNNING THE REFERENCE ITSELF on the CPU (build container
only; needs the reference checkout that _ref_loader.py names).  Only arrays, seeds and strings are stored.

    python tests/golden/make_itc_golden.py [--skip-large]

  itc_small.npz   small geometry (config.blip_itm_small(64)), B = 3 images, 3 ragged captions of which one is a single word
                  (an L = 3 row): sim of forward(match_head="itc"), and the five fields of extract_features in its three modes
  itc_large.npz   BLIP-ITM-large 336^2, B = 2, T = 2: sim, the CLS-row features of both sides, and the first 8 tokens of every
                  all-token array (the committed-file size limit)

The reference's extract_features ends in `BlipOutputFeatures(...)`, a name its file never imports: the generator puts a
namedtuple of that name (a stand-in of ours, five fields) into the loaded module's globals.  The projections vision_proj /
text_proj are filled from synth.itc_state_dict (same seed as the other weights).
"""
import argparse
import collections
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "pnp-ovss_amd"))
sys.path.insert(0, HERE)

from pnp_ovss import config as C            # noqa: E402
from pnp_ovss import synth                  # noqa: E402
from pnp_ovss.tokenizer import SynthTokenizer  # noqa: E402
import _ref_loader as RL                    # noqa: E402

FIELDS = ("image_embeds", "image_embeds_proj", "text_embeds", "text_embeds_proj", "multimodal_embeds")
BlipOutputFeatures = collections.namedtuple("BlipOutputFeatures", FIELDS)


def _model(cfg, seed):
    tok = SynthTokenizer(cfg.vocab)
    sd = synth.synth_state_dict(cfg, seed)
    sd.update(synth.itc_state_dict(cfg, seed))
    m, itm = RL.build_reference_model(cfg, sd, tok)
    for n, a in synth.itc_state_dict(cfg, seed).items():          # loaded, not left at their random initialisation
        assert np.array_equal(m.state_dict()[n].numpy(), a), n
    itm.BlipOutputFeatures = BlipOutputFeatures
    return m, tok


def _run(cfg, weight_seed, image_seed, caps):
    m, tok = _model(cfg, weight_seed)
    _, imgs = synth.synth_images(len(caps), cfg.img_size, seed=image_seed)
    samples = {"image": torch.from_numpy(imgs), "text_input": list(caps)}
    out = {}
    with torch.no_grad():
        out["sim"] = m(samples, match_head="itc").numpy()
        for mode in ("image", "text", "multimodal"):
            f = m.extract_features(samples, mode=mode)
            for k in FIELDS:
                v = getattr(f, k)
                out[f"{mode}__{k}"] = None if v is None else v.numpy()
    enc = tok(list(caps), padding="longest", truncation=True, max_length=500, return_tensors="pt")
    return out, enc


def gen_itc_small():
    cfg = C.blip_itm_small(64)
    caps = ["A picture of cat aeroplane dog", "bus", "A picture of person tvmonitor sheep boat"]
    out, enc = _run(cfg, 3, 5, caps)
    assert int(enc.attention_mask.sum(1).min()) == 3            # the single-word caption: [CLS] bus [SEP]
    arrays = {k: v for k, v in out.items() if v is not None}
    np.savez_compressed(os.path.join(HERE, "itc_small.npz"), cfg=json.dumps(cfg.as_dict()), weight_seed=3, image_seed=5,
                        captions=np.array(caps), input_ids=enc.input_ids.numpy(), attention_mask=enc.attention_mask.numpy(),
                        none_fields=np.array(sorted(k for k, v in out.items() if v is None)), **arrays)
    print("itc_small:", {k: v.shape for k, v in arrays.items()}, "sim", out["sim"])


def gen_itc_large():
    cfg = C.blip_itm_large(336)
    caps = ["A picture of cat dog", "bus"]
    out, enc = _run(cfg, 0, 1234, caps)
    arrays = {"sim": out["sim"],
              "image_cls_proj": out["image__image_embeds_proj"][:, 0],
              "text_cls_proj": out["text__text_embeds_proj"][:, 0]}
    for k, v in out.items():
        if v is not None and k != "sim":
            arrays[k + "__first8"] = np.ascontiguousarray(v[:, :8])
    np.savez_compressed(os.path.join(HERE, "itc_large.npz"), cfg=json.dumps(cfg.as_dict()), weight_seed=0, image_seed=1234,
                        captions=np.array(caps), input_ids=enc.input_ids.numpy(), attention_mask=enc.attention_mask.numpy(),
                        none_fields=np.array(sorted(k for k, v in out.items() if v is None)), **arrays)
    print("itc_large:", {k: v.shape for k, v in arrays.items()}, "sim", out["sim"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    gen_itc_small()
    if not a.skip_large:
        gen_itc_large()
