// C ABI over the reference's own pixel shaders (test infrastructure only).  `make -C oracle ref` appends this file to the piped effect
// text: by then namespace ref_cas holds cas.effect with its FidelityFX includes and namespace ref_fsr holds fsr.effect with its own.
// The driver sets the effects' uniforms, walks the output pixels and calls PSMain / EASUPSMain with the texture coordinate of the
// pixel centre, uv = ((x + 0.5) / ow, (y + 0.5) / oh) in float32; the shader's own floor(uv * output_size) has to give (x, y) back,
// which is checked for every pixel.  Returns 0, or -1 for bad arguments, or -2 where that check fails.

extern "C" int ffx_ref_cas_unit(const float* frame, int rows, int cols, float peak, float* out)
{
    using namespace ffx_shim;
    if (!frame || !out || rows <= 0 || cols <= 0) return -1;
    ref_cas::image = texture2d(frame, frame + 1, frame + 2, 3, cols, rows);
    ref_cas::output_size = float2((float)cols, (float)rows);
    ref_cas::cas_const_1 = float4(peak, 0.0f, 0.0f, 0.0f);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            ref_cas::VSData vs;
            vs.uv = float2(((float)x + 0.5f) / (float)cols, ((float)y + 0.5f) / (float)rows);
            if (floorf(vs.uv.x * (float)cols) != (float)x || floorf(vs.uv.y * (float)rows) != (float)y) return -2;
            const float4 c = ref_cas::PSMain(vs);
            float* o = out + ((long)y * cols + x) * 4;
            o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w;
        }
    return 0;
}

// r, g, b: float32 [H, W] planes; region = (x, y, w, h); con: the 16 words of FsrEasuCon; out: float32 [oh, ow, 4] (r, g, b, a);
// sample_dev: the largest distance of a sampled u W or v H from a texel centre k + 0.5.  region_uv_offset is the quotient the plugin's
// FSREffect::configure passes, (x / W, y / H) in float32.
extern "C" int ffx_ref_easu_unit(const float* r, const float* g, const float* b, int W, int H, const int* region, int ow, int oh,
                                 const float* con, float* out, float* sample_dev)
{
    using namespace ffx_shim;
    if (!r || !g || !b || !region || !con || !out || W <= 0 || H <= 0 || ow <= 0 || oh <= 0) return -1;
    ref_fsr::image = texture2d(r, g, b, 1, W, H);
    ref_fsr::input_size = float2((float)W, (float)H);
    ref_fsr::output_size = float2((float)ow, (float)oh);
    ref_fsr::region_uv_offset = float2((float)region[0] / (float)W, (float)region[1] / (float)H);
    ref_fsr::easu_const_0 = float4(con[0], con[1], con[2], con[3]);
    ref_fsr::easu_const_1 = float4(con[4], con[5], con[6], con[7]);
    ref_fsr::easu_const_2 = float4(con[8], con[9], con[10], con[11]);
    ref_fsr::easu_const_3 = float4(con[12], con[13], con[14], con[15]);
    g_sample_dev = 0.0f;
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            ref_fsr::VSData vs;
            vs.uv = float2(((float)x + 0.5f) / (float)ow, ((float)y + 0.5f) / (float)oh);
            if (floorf(vs.uv.x * (float)ow) != (float)x || floorf(vs.uv.y * (float)oh) != (float)y) return -2;
            const float4 c = ref_fsr::EASUPSMain(vs);
            float* o = out + ((long)y * ow + x) * 4;
            o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w;
        }
    if (sample_dev) *sample_dev = g_sample_dev;
    return 0;
}
