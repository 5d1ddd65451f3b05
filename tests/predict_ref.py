"""CPU restatement of the reference's inference outputs -- the parity pin of iswm_amd/csrc/predict.hip and
iswm_amd/predict.py.

numpy + torch (CPU) only.  Line numbers cite the reference's predict.py.  The reference runs these steps on float32
tensors and arrays; the restatement keeps every dtype it uses, so that threshold compares, the uint8 truncation and
the fp64 band compare are the reference's own.
"""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)      # get_transform, :93-97
STD = (0.229, 0.224, 0.225)


def normalize(img_u8):
    """T.ToTensor() then T.Normalize(mean, std) (:93-97) on a uint8 [H, W, 3] image -> fp32 [3, H, W]:
    ToTensor divides the float32 image by 255, Normalize subtracts and divides channel-wise in float32"""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1).float().div(255)
    m = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(STD, dtype=torch.float32)[:, None, None]
    return x.sub(m).div(s)


def softmax_fg(logits, fg=1):
    """torch.softmax(logits, dim=1)[:, fg] (:264-267) evaluated in fp64 on [N, C, H, W] logits"""
    lg = np.asarray(logits, dtype=np.float64)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return e[:, fg] / e.sum(axis=1)


def predict_mask(prob_fg, threshold):
    """the maps of predict_mask (:258-290) from the foreground probability: the reference holds it as float32, so it
    is rounded to float32 first.
      pred = (prob > threshold) -> 0 / 255 (:275, decoded to 0 / 255: this project's decode_target); the compare of
             a float32 tensor with a Python float is done in float32;
      conf = (prob * 255).astype(np.uint8) (:287-288): a float32 product, truncated;
      stats = (min, max, mean, fraction below threshold) as printed at :271-272 (numpy float32 array against a
             Python float: a float32 compare)."""
    p = np.asarray(prob_fg, dtype=np.float32)
    thr32 = np.float32(threshold)
    pred = np.where(p > thr32, 255, 0).astype(np.uint8)
    conf = (p * np.float32(255)).astype(np.uint8)
    return pred, conf


def prob_stats(prob_fg, threshold):
    """(min, max, sum, count(p < thr), count(p > thr)) of one float32 probability map, fp64 sum"""
    p = np.asarray(prob_fg, dtype=np.float32)
    thr32 = np.float32(threshold)
    return (float(p.min()), float(p.max()), float(p.astype(np.float64).sum()), int((p < thr32).sum()),
            int((p > thr32).sum()))


def binarize_confidence_map(conf, min_prob=0.2, max_prob=0.7):
    """binarize_confidence_map without wave processing (:227-234): conf / 255.0 in fp64, 255 where
    min_prob <= it <= max_prob"""
    c = np.asarray(conf)
    prob = c / 255.0
    out = np.zeros_like(c, dtype=np.uint8)
    out[(prob >= min_prob) & (prob <= max_prob)] = 255
    return out


def has_internal_wave(pred_mask, area_threshold=0.01):
    """:99-125 on a grey-level mask: foreground = mask > 127; True when its area ratio exceeds the threshold.
    Returns (ratio, decision)."""
    m = np.asarray(pred_mask)
    fg = np.all(m == [255, 255, 255], axis=2) if (m.ndim == 3 and m.shape[2] == 3) else m > 127
    ratio = np.sum(fg) / fg.size
    return ratio, ratio > area_threshold


def near_boundary(prob64, threshold, eps):
    """pixels whose fp64 probability lies within eps of a decision of the restatement: the threshold, an integer of
    p * 255 (conf's truncation, and with it the band, which depends on conf alone)"""
    p = np.asarray(prob64, dtype=np.float64)
    q = p * 255.0
    return (np.abs(p - threshold) <= eps) | (np.abs(q - np.round(q)) <= 255.0 * eps)
