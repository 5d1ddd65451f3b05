"""CPU restatement of the reference's save_validation_results panels (train.py:461-523) -- the parity pin of
iswm_amd/csrc/val_panels.hip and iswm_amd/val_results.py.

numpy + torch (CPU) only.  Line numbers cite the reference's train.py and utils/utils.py.  Every dtype is the
reference's: the denormalisation constants are fp64 quotients cast to float32 by torchvision's normalize, the image
arithmetic is float32, the probability is restated in fp64 and its truncation in float32.
"""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)      # train.py:491
STD = (0.229, 0.224, 0.225)


def denorm_constants(mean=MEAN, std=STD):
    """Denormalize.__init__ (utils/utils.py:15-19): _mean = -mean / std, _std = 1 / std in fp64; normalize() then
    builds float32 tensors from them (torch.as_tensor(..., dtype=tensor.dtype))"""
    mean, std = np.array(mean), np.array(std)
    return torch.as_tensor(-mean / std, dtype=torch.float32), torch.as_tensor(1 / std, dtype=torch.float32)


def denormalize_f32(x):
    """Denormalize(mean, std)(x) * 255 (utils/utils.py:21-24, train.py:491-492) on a float32 [3, H, W] tensor ->
    float32 [H, W, 3]: tensor.sub(_mean).div(_std), then * 255, all float32"""
    m, s = denorm_constants()
    t = torch.as_tensor(x, dtype=torch.float32).sub(m[:, None, None]).div(s[:, None, None])
    return (t * 255).permute(1, 2, 0).numpy()


def denormalize_u8(x):
    """.astype(np.uint8) of denormalize_f32 (train.py:492): truncation toward zero for 0 <= t < 256, which is every
    value a uint8 image gives.  Outside that range numpy wraps around; the kernel clamps instead (t < 0 or NaN -> 0,
    t > 255 -> 255), and so does this function"""
    t = denormalize_f32(x)
    with np.errstate(invalid="ignore"):
        inside = (t >= 0) & (t <= 255)
        out = np.where(inside, t, 0).astype(np.uint8)
        out[t > 255] = 255
    return out


def decode_target(target, num_classes=2):
    """train.py:611-618, verbatim in behaviour: white where the mask is 1 for num_classes == 2, black everywhere else
    and for every other class count"""
    target = np.array(target)
    rgb = np.zeros((target.shape[0], target.shape[1], 3), dtype=np.uint8)
    if num_classes == 2:
        rgb[target == 1] = [255, 255, 255]
    return rgb


def palette(num_classes):
    """256 x 3 colours by class index: decode_target for num_classes == 2; otherwise the PASCAL VOC colour map (bit k
    of the index's octal digit j goes to bit 7 - j of channel k), which this project paints where the reference paints
    black"""
    pal = np.zeros((256, 3), dtype=np.uint8)
    if num_classes == 2:
        pal[1] = 255
        return pal
    for i in range(256):
        r = g = b = 0
        c = i
        for j in range(8):
            r |= (c & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[i] = (r, g, b)
    return pal


def max_prob(logits):
    """torch.max(F.softmax(logits, dim=1), dim=1)[0] (train.py:494-495) in fp64 on [N, C, H, W] logits:
    1 / sum_c exp(l_c - max l)"""
    lg = np.asarray(logits, dtype=np.float64)
    return 1.0 / np.exp(lg - lg.max(axis=1, keepdims=True)).sum(axis=1)


def conf_u8(prob):
    """(conf * 255).clip(0, 255).astype(np.uint8) (train.py:515); the reference holds conf as float32, so it is
    rounded to float32 first and the product is a float32 product"""
    p = np.asarray(prob, dtype=np.float32)
    return (p * np.float32(255)).clip(0, 255).astype(np.uint8)


def near_boundary(prob64, eps):
    """pixels whose fp64 probability lies within eps of an integer of p * 255, conf's only decision"""
    q = np.asarray(prob64, dtype=np.float64) * 255.0
    return np.abs(q - np.round(q)) <= 255.0 * eps


def overlay(original, pred_rgb):
    """the 0.7-alpha composite the reference asks matplotlib for (train.py:508-513: imshow(original), then
    imshow(pred_rgb, alpha=0.7)) at native resolution, in integers with round-half-up: (3 o + 7 p + 5) // 10"""
    o, p = np.asarray(original).astype(np.int64), np.asarray(pred_rgb).astype(np.int64)
    return ((3 * o + 7 * p + 5) // 10).astype(np.uint8)


GREY, BLACK, WHITE, RED, BLUE, MAGENTA = (128, 128, 128), (0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255), (255, 0, 255)


def error_map(label, pred):
    """the error panel (this project's, no counterpart in the reference), per pixel in this order: label 255 grey;
    pred == label black on background / white on foreground; label 0 with a foreground pred red; a foreground label
    with pred 0 blue; two different foreground classes magenta"""
    label, pred = np.asarray(label).astype(np.int64), np.asarray(pred).astype(np.int64)
    out = np.empty(label.shape + (3,), dtype=np.uint8)
    out[...] = MAGENTA
    out[(label != 0) & (pred == 0)] = BLUE
    out[(label == 0) & (pred != 0)] = RED
    out[(pred == label) & (label != 0)] = WHITE
    out[(pred == label) & (label == 0)] = BLACK
    out[label == 255] = GREY
    return out
