from .image_metrics import ImageMetricModule, LPIPSModule, PSNRModule, SSIMModule, image_quality, image_quality_stats
from .metrics import (calculate_accuracy, calculate_f1_score, calculate_lpips, calculate_precision, calculate_psnr, calculate_recall,
                      calculate_ssim)
