"""Scores of the failure-replay confusion matrix (label 1 = failure) and the image metrics as plain functions: the interface of the
reference's uncertainty/evaluation/metrics.py.  y_true and y_pred are numpy arrays of 0 / 1 labels.  The scores are the textbook
ratios on numpy integers, so an empty denominator gives numpy's 0 / 0 -- NaN with a RuntimeWarning -- and is not guarded away."""
import numpy as np

from .image_metrics import LPIPSModule, PSNRModule, SSIMModule


def _confusion(y_true, y_pred):
    """(true positives, false positives, false negatives)"""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    hit = y_pred == 1
    return np.sum(hit & (y_true == 1)), np.sum(hit & (y_true == 0)), np.sum((y_pred == 0) & (y_true == 1))


def calculate_accuracy(y_true, y_pred):
    return np.mean(np.asarray(y_true) == np.asarray(y_pred))


def calculate_precision(y_true, y_pred):
    tp, fp, _ = _confusion(y_true, y_pred)
    return tp / (tp + fp)


def calculate_recall(y_true, y_pred):
    tp, _, fn = _confusion(y_true, y_pred)
    return tp / (tp + fn)


def calculate_f1_score(y_true, y_pred):
    p, r = calculate_precision(y_true, y_pred), calculate_recall(y_true, y_pred)
    return 2 * (p * r) / (p + r)


def calculate_psnr(preds, target, mask=None):
    return PSNRModule()(preds, target, mask)


def calculate_ssim(preds, target, mask=None):
    return SSIMModule()(preds, target, mask)


def calculate_lpips(preds, target, mask=None):
    return LPIPSModule()(preds, target, mask)
