"""shim for the reference import path SR.psnr_ssim: the three tensor metrics (calculate_psnr_pt / calculate_ssim_pt / calculate_cpsnr_pt).
None of the reference module's top-level imports (cv2, clip, open_clip, lpips) is needed; its numpy / cv2 variants and the CLIP / LPIPS
scores stay with the caller."""
from srbh_amd.sr_metrics import calculate_cpsnr_pt, calculate_psnr_pt, calculate_ssim_pt  # noqa: F401
