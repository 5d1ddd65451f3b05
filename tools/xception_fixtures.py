"""Records tests/golden/xception_keys.json and tests/golden/xception_features.npz from a checkout of the reference project.

    python tools/xception_fixtures.py /path/to/reference

xception_keys.json: [[name, shape], ...] of the state_dict of the reference's Xception (replace_stride_with_dilation
[False, False, False, True]: output stride 16) behind the reference's IntermediateLayerGetter with return_layers
{'conv4': 'out', 'block1': 'low_level'}, in order.
xception_features.npz: `input` [1, 3, 131, 99] and the features `out` / `low_level` of that module in eval mode, float64
arithmetic stored as float32, with the weights tests/xception_ref.numpy_state(keys, FIXTURE_SEED) gives.

The reference is imported by path; nothing of it is copied.  No test runs this script."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_SEED = 1


def main(ref_root):
    sys.path.insert(0, ROOT)
    from tests import xception_ref as R
    sys.path.insert(0, ref_root)
    from network.backbone.xception import Xception
    from network.utils import IntermediateLayerGetter
    m = IntermediateLayerGetter(Xception(replace_stride_with_dilation=[False, False, False, True]),
                                return_layers={'conv4': 'out', 'block1': 'low_level'})
    entries = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "xception_keys.json"), "w") as f:
        json.dump(entries, f, indent=0)
        f.write("\n")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.numpy_state(entries, FIXTURE_SEED).items()}, strict=True)
    m = m.double().eval()
    x = R.synth_images(1, 131, 99, FIXTURE_SEED)
    with torch.no_grad():
        feats = m(x.double())
    np.savez_compressed(os.path.join(golden, "xception_features.npz"), input=x.numpy(),
                        out=feats['out'].float().numpy(), low_level=feats['low_level'].float().numpy())
    print(len(entries), {k: tuple(v.shape) for k, v in feats.items()})


if __name__ == "__main__":
    main(sys.argv[1])
