"""Golden vectors of the question injected at g layers 1 and 3, recorded from the REFERENCE itself.

Run in the build container only (make_golden imports the reference's model.py):   python tests/golden/make_golden_inject.py

The reference's CLI moves the question with `--question-injection N` (its train.py overrides
`question_injection_position` in the hyperparameters); these fixtures do the same to the ir-fp
hyperparameters and record RelationalLayers built from them, with make_golden's recorder:
  G-inj{1,3}-small  B = 2,  n = 64, strided objects, full pair rows and all gradients (like G-ir-small)
  G-inj{1,3}-64     B = 64, n = 64                                                      (like G-ir64)
`meta` carries the base config and the injection position ("inject"), so a test rebuilds hyp without a table entry.
Writes only these four files."""
import json
import os

import numpy as np

import make_golden as mg

POSITIONS = (1, 3)
BASE = "ir-fp"


def hyp_at(position):
    return dict(mg.REF_HYP[BASE], question_injection_position=position)


def add_meta(tag, position):
    path = os.path.join(mg.HERE, tag + ".npz")
    with np.load(path) as z:
        out = {k: z[k] for k in z.files}
    meta = json.loads(str(out["meta"]))
    meta.update(base_cfg=BASE, inject=position)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    for p in POSITIONS:
        cfg = "%s@%d" % (BASE, p)
        mg.REF_HYP[cfg] = hyp_at(p)                  # (formula.formula_rl_state sizes the layers from hyp)
    for p, seed_small, seed_64 in ((1, 23, 42), (3, 24, 43)):
        cfg = "%s@%d" % (BASE, p)
        mg.record_rl("G-inj%d-small" % p, cfg, 2, 64, seed=seed_small, strided=True, full=True, full_grads=True)
        add_meta("G-inj%d-small" % p, p)
        mg.record_rl("G-inj%d-64" % p, cfg, 64, 64, seed=seed_64)
        add_meta("G-inj%d-64" % p, p)
