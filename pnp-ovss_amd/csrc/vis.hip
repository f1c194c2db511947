// Colour overlay of a label map on its image, on gfx950: the reference's Draw_Segmentation_map (PnP_OVSS_0514_updated_
// segmentation_coco.py:966-983) calls skimage.color.label2rgb(kind="overlay", alpha=0.3, bg_label=0, image_alpha=1,
// saturation=0) and matplotlib's imsave turns the float image into bytes.  Restated here in double precision, in this order
// (this translation unit is compiled with -ffp-contract=off, so every product and sum below rounds on its own, as numpy's do):
//     g     = ((0.2125 * R + 0.7154 * G) + 0.0721 * B) / 255
//     l = 0 : out_c = uint8(g * 255)                                          (the grey image; truncation)
//     l > 0 : out_c = uint8(((pal[l][c] / 255) * alpha + g * (1 - alpha)) * 255)
// The palette is indexed by the label itself (the reference colours by the label's rank among those present in an image).
//   overlay_labels_kernel   one thread per pixel of the concatenated batch, grid-stride.  Labels, RGB and the output use the
//                           same pixel numbering (byte 3p of the HWC buffers belongs to pixel p of the label buffer), so the
//                           kernel needs only the pixel total d_pix_off[B], which it reads on the device: no host read-back.
#include "common.h"
#include "kernels.h"

namespace pnp {

__global__ __launch_bounds__(256) void overlay_labels_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ rgb,
                                                             const int64_t* __restrict__ pix_off, int B,
                                                             const uint8_t* __restrict__ palette, double alpha,
                                                             uint8_t* __restrict__ out) {
    const int64_t n = pix_off[B];
    const double beta = 1.0 - alpha;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int l = labels[p];
        const double r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
        const double grey = (0.2125 * r + 0.7154 * g + 0.0721 * b) / 255.0;
        double v[3];
        if (l == 0) {
            v[0] = v[1] = v[2] = grey * 255.0;
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = (((double)palette[3 * l + c] / 255.0) * alpha + grey * beta) * 255.0;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) out[3 * p + c] = (uint8_t)(int)fmin(fmax(v[c], 0.0), 255.0);
    }
}

}  // namespace pnp

extern "C" int pnp_overlay_labels(const uint8_t* d_labels, const uint8_t* d_rgb, const int64_t* d_pix_off, int32_t B,
                                  const uint8_t* d_palette, double alpha, uint8_t* d_out, void* stream) {
    if (!d_labels || !d_rgb || !d_pix_off || !d_palette || !d_out || B < 1 || !(alpha >= 0.0 && alpha <= 1.0)) return PNP_ERR_ARG;
    hipLaunchKernelGGL(pnp::overlay_labels_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, d_labels, d_rgb, d_pix_off, (int)B,
                       d_palette, alpha, d_out);
    return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP;
}
