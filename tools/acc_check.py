"""whole-model train-mode logits of this path vs (a) the reference's golden vector (torch CPU fp32) and (b) the oracle
evaluated in float64 -- separates this path's own rounding error from the reference's (inputs: oracle/make_golden.py MODEL_INPUT)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from tests.util import load, rel_err
from iswm_amd import ops
from iswm_amd.network import modeling
from oracle.deeplab import OracleDeepLab
from oracle.make_golden import model_input, model_state
from oracle.synth import ArchCfg, synth_state_dict

for planes, (tag, backbone, os_) in [(p, c) for c in (("r50_os16", "resnet50", 16), ("r101_os8", "resnet101", 8))
                                     for p in (True, False)]:
    ops._PLANES_ENV = planes          # False: every activation fp32 (the round-1 data path)
    fx = load("model_%s.npz" % tag)
    cfg = ArchCfg("deeplabv3plus", backbone, 2, os_)
    sd = model_state(tag, cfg)
    x = model_input(tag)[0]
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    o64 = OracleDeepLab(cfg, sd64, dropout_p=0.0).train()
    with torch.no_grad():
        ref64 = o64(x.double())
    m = modeling._segm_resnet("deeplabv3plus", backbone, 2, os_, False)
    m.load_state_dict(sd, strict=True)
    m.classifier.aspp.project[3].p = 0.0
    m = m.cuda().train()
    with torch.no_grad():
        lg = m(x.cuda())
    print("%s planes=%s: vs golden(fp32 cpu) %.3e   vs oracle fp64 %.3e   golden vs fp64 %.3e" %
          (tag, int(planes), rel_err(lg, fx["train_logits"]), rel_err(lg, ref64), rel_err(fx["train_logits"], ref64)))
