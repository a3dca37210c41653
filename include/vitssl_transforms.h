/*
 * vitssl_transforms.h -- C ABI of the fused input-transform kernel of libvitssl_hip.so (MI355X, gfx950).
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers owned by the caller; enqueued on `stream`, never synchronised).  Kept in a header of its own so that
 * the symbol list of vitssl_hip.h and vitssl_version() stay what they are; the Python mirror binds these through
 * vitssl_hip._lib.REGISTRY["transforms"].
 */
#ifndef VITSSL_TRANSFORMS_H
#define VITSSL_TRANSFORMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- SimMIM / supervised / finetune / eval transform lists ---------------------------------
 * Replaces, per image, the torchvision lists that utils/train_utils.py:54-68 builds and the datasets apply on the CPU
 * with PIL images:
 *   configs/{simmim,supervised,finetune}/train_transforms.yaml = RandomResizedCrop(size, scale [0.9, 1.0]),
 *                                                                RandomHorizontalFlip, ToTensor
 *   configs/{simmim,supervised,finetune}/val_transforms.yaml, configs/unsupervised_eval/transforms.yaml,
 *   configs/supervised_eval/transforms.yaml                    = Resize([h, w]), ToTensor
 * One launch: crop box -> Pillow BILINEAR resize (horizontal 8-bit pass rounded to uint8, then vertical 8-bit pass; the
 * filter support widens when downscaling) -> optional horizontal flip -> ToTensor (/255, channel-first).  The
 * horizontally resampled rows of an output-row tile live in LDS as uint8; nothing but `src` is read from and nothing but
 * `out` is written to device memory.  Bit-identical to Pillow (oracle/augment_oracle.py: resized_crop_u8 + to_tensor);
 * the fixed-point taps are the ones vitssl_aug_resized_crop_u8 uses (csrc/resample_taps.h).
 *   src     u8    [B, H, W, 3]
 *   iparams int32 [B, 5] = top, left, h, w, flip     (drawn on the host, vit-ssl_amd/data/transforms.py; Resize is the
 *                                                      full-image box 0, 0, H, W with flip 0)
 *   out     f32   [B, 3, SH, SW]
 * Every box must lie inside its image (0 <= top, top + h <= H, 0 <= left, left + w <= W, h, w >= 1): the caller's
 * contract, as for vitssl_aug_resized_crop_u8.
 * Limits (VITSSL_ERR_ARG beyond them, the message names the limit): the LDS rows of ONE output row -- 2 * max(H / SH, 1)
 * + 2 rows of SW pixels -- together with the tap tables must fit 64 KiB; H, W < 2^23; ceil(W / SW) and ceil(H / SH) <=
 * 127.  Inside that range the output-row tile (32 ... 1 rows) is chosen per shape so that the rows fit: 32x32 and 96x96
 * sources to 224x224, 512x512 to 96x96 and 600x600 to 512x512 all are. */
int vitssl_tf_resized_crop_to_tensor(const uint8_t* src, const int32_t* iparams, float* out, int B, int H, int W, int SH,
                                     int SW, void* stream);
/* introspection for tests and tools, like the vitssl_debug_* getters of vitssl_hip.h (launches nothing): output rows per
 * workgroup tile the call above uses for this shape (> 0), or VITSSL_ERR_ARG where it refuses the shape; the launch has
 * B * ceil(SH / rows) workgroups */
int vitssl_debug_tf_tile_rows(int H, int W, int SH, int SW);

#ifdef __cplusplus
}
#endif
#endif
