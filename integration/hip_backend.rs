//! src/hip_backend.rs for zlogic/matrix-eyes: the safe layer over hip_ffi.rs that `reconstruction::extract_depth`
//! calls under `#[cfg(feature = "hip")]` in place of `DepthProModelLoader::extract_depth::<B>` + `DepthMap::new::<B>`
//! (reconstruction.rs:155-205).  NOT COMPILED in the build image (no Rust toolchain there); the compiled twin
//! of this file is matrix-eyes_amd/host/matrix_eyes.{hpp,cpp}, function for function.
#![cfg(feature = "hip")]
use crate::hip_ffi as ffi;
use std::ffi::{c_char, c_void, CStr, CString};
use std::ptr::{null, null_mut};

#[derive(Debug)]
pub struct HipError {
    pub code: i32,
    pub message: String,
}
impl std::fmt::Display for HipError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "HIP back end error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for HipError {}

/// reconstruction::init_device (reconstruction.rs:42-72): one context = one GPU, one stream, resident weights.
pub struct HipDevice {
    ctx: *mut ffi::MeCtx,
    weights_loaded: std::cell::Cell<bool>,
}

impl HipDevice {
    pub fn new(device_id: i32) -> Result<HipDevice, HipError> {
        let mut ctx: *mut ffi::MeCtx = null_mut();
        let rc = unsafe { ffi::me_ctx_create(device_id, ffi::ME_DTYPE_F16, null(), &mut ctx) };
        if rc != ffi::ME_OK {
            return Err(last_error(null(), rc));
        }
        Ok(HipDevice { ctx, weights_loaded: std::cell::Cell::new(false) })
    }

    /// A loop over many images (main.rs called per file of a batch): `.obj` files are written behind the caller by up
    /// to `files_in_flight` host threads while the GPU works on the next image; `flush_outputs` before the files are
    /// read.  0 restores the reference's form (output_mesh returns with the file written).
    pub fn set_write_behind(&self, files_in_flight: i32) -> Result<(), HipError> {
        self.check(unsafe { ffi::me_ctx_set_write_behind(self.ctx, files_in_flight) })
    }

    /// Waits for every file a write-behind `output_mesh` has handed to a host thread; a failed write surfaces here
    /// (or at the next `output_mesh` that has to wait for it) as the OutputError::Io it would have been.
    pub fn flush_outputs(&self) -> Result<(), HipError> {
        self.check(unsafe { ffi::me_output_flush(self.ctx) })
    }

    /// RgbImage::save to ".png" for any 8-bit RGB picture (host bytes): encoded on the GPU, written to `destination_path`
    pub fn save_png(&self, rgb: &[u8], w: u32, h: u32, destination_path: &str) -> Result<(), HipError> {
        assert_eq!(rgb.len(), w as usize * h as usize * 3);
        let dst = CString::new(destination_path).unwrap();
        self.check(unsafe { ffi::me_output_png(self.ctx, rgb.as_ptr(), w as i32, h as i32, dst.as_ptr()) })
    }

    /// RgbImage::save to ".jpg" / ".jpeg" for any 8-bit RGB picture (host bytes): a baseline JPEG encoded on the GPU with
    /// libjpeg's bytes for `quality` (1..100) and `subsampling` (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), written to `destination_path`
    pub fn save_jpeg(&self, rgb: &[u8], w: u32, h: u32, quality: i32, subsampling: i32, destination_path: &str) -> Result<(), HipError> {
        assert_eq!(rgb.len(), w as usize * h as usize * 3);
        let dst = CString::new(destination_path).unwrap();
        self.check(unsafe { ffi::me_output_jpeg(self.ctx, rgb.as_ptr(), w as i32, h as i32, quality, subsampling, dst.as_ptr()) })
    }

    /// DynamicImage::resize_exact(nw, nh, FilterType::Lanczos3) for an RGB8 buffer (reconstruction.rs:107-113,
    /// output.rs:206-218) on the GPU: the bytes `image` 0.25.10 writes.  `rgb` is `[h, w, 3]`, the result `[nh, nw, 3]`.
    pub fn resize_exact_lanczos3(&self, rgb: &[u8], w: u32, h: u32, nw: u32, nh: u32) -> Result<Vec<u8>, HipError> {
        assert_eq!(rgb.len(), w as usize * h as usize * 3);
        let mut out = vec![0u8; nw as usize * nh as usize * 3];
        self.check(unsafe { ffi::me_resize_lanczos3_rgb8(self.ctx, rgb.as_ptr(), w as i32, h as i32, out.as_mut_ptr(), nw as i32, nh as i32) })?;
        Ok(out)
    }

    /// reconstruction.rs:95-113 for a JPEG photo in one call, in place of `ImageReader::open(..).decode()`,
    /// `apply_orientation` and `resize_exact(IMG_SIZE, IMG_SIZE, Lanczos3)`: `file` is the file's bytes, `orientation` the
    /// EXIF value (1..8) the caller read from the block `jpeg_info` points at.  Entropy decoding runs on the host, the
    /// reconstruction, the orientation and the resize on the GPU; only the `[nh, nw, 3]` picture comes back.  The pixels are
    /// the C++ host layer's decoder's, which agrees with `image`'s (zune-jpeg) to within JPEG's usual unit or two.
    pub fn decode_jpeg_resized(&self, file: &[u8], orientation: i32, nw: u32, nh: u32) -> Result<Vec<u8>, HipError> {
        let mut out = vec![0u8; nw as usize * nh as usize * 3];
        self.check(unsafe { ffi::me_jpeg_decode_resized_rgb8(self.ctx, file.as_ptr(), file.len() as i64, orientation, out.as_mut_ptr(), nw as i32, nh as i32) })?;
        Ok(out)
    }

    /// Where `decode_jpeg_resized` runs the Huffman decoding: `false` (the default) on the host, `true` on the GPU
    /// (`me_ctx_set_jpeg_entropy`; sequential single-scan files -- anything else falls back to the host loop).  The same pixels.
    pub fn set_jpeg_entropy_on_device(&self, on: bool) -> Result<(), HipError> {
        self.check(unsafe { ffi::me_ctx_set_jpeg_entropy(self.ctx, on as i32) })
    }

    /// (width, height, exif_offset, exif_len) of a JPEG file: the size as coded and where its TIFF-structured EXIF block
    /// lies in `file` (0, 0: none) -- hand that slice to `exif::Reader::read_raw`.  No GPU work.
    pub fn jpeg_info(file: &[u8]) -> Result<(u32, u32, usize, usize), HipError> {
        let (mut w, mut h, mut off, mut n) = (0i32, 0i32, 0i64, 0i64);
        let rc = unsafe { ffi::me_jpeg_info(file.as_ptr(), file.len() as i64, &mut w, &mut h, &mut off, &mut n) };
        if rc != ffi::ME_OK {
            return Err(last_error(std::ptr::null(), rc));
        }
        Ok((w as u32, h as u32, off as usize, n as usize))
    }

    fn check(&self, rc: i32) -> Result<(), HipError> {
        if rc == ffi::ME_OK {
            Ok(())
        } else {
            Err(last_error(self.ctx, rc))
        }
    }

    /// mod.rs:174-249 load_record, once per device: the library reads the PyTorch archive itself (no key remap,
    /// no transpose adapter: it takes PyTorch names and layouts).  mod.rs:211-247: a valid `.mearena` cache beside the
    /// checkpoint is loaded instead, and written after loading when `convert_checkpoints` is set.
    pub fn ensure_loaded(&self, checkpoint_path: &str, convert_checkpoints: bool) -> Result<(), HipError> {
        if self.weights_loaded.get() {
            return Ok(());
        }
        let path = CString::new(checkpoint_path).map_err(|_| HipError { code: ffi::ME_ERR_BAD_ARG, message: "path".into() })?;
        self.check(unsafe { ffi::me_load_checkpoint_cached(self.ctx, path.as_ptr(), convert_checkpoints as i32, std::ptr::null_mut()) })?;
        self.weights_loaded.set(true);
        Ok(())
    }

    /// mod.rs:251-363 extract_depth on the u8 HWC pixels of SourceImage::load (reconstruction.rs:114): the
    /// normalise / permute of :116-124 runs on the GPU.  f_norm None = FOV head (mod.rs:343-358).
    pub fn extract_depth_u8<PL: crate::depth_pro::ProgressListener>(
        &self, rgb8: &[u8], size: usize, f_norm: Option<f32>, pl: Option<PL>,
    ) -> Result<Vec<f32>, HipError> {
        assert_eq!(rgb8.len(), size * size * 3);
        let mut depth = vec![0f32; size * size];
        let mut boxed = pl;
        unsafe extern "C" fn trampoline<PL: crate::depth_pro::ProgressListener>(user: *mut c_void, pos: f32, msg: *const c_char) {
            let pl = &*(user as *const PL);
            pl.report_status(pos);
            if !msg.is_null() {
                pl.update_message(CStr::from_ptr(msg).to_string_lossy().into_owned());
            }
        }
        if let Some(p) = boxed.as_mut() {
            self.check(unsafe { ffi::me_ctx_set_progress(self.ctx, Some(trampoline::<PL>), p as *mut PL as *mut c_void) })?;
        }
        let fn_ptr = f_norm.as_ref().map_or(null(), |f| f as *const f32);
        let rc = unsafe { ffi::me_extract_depth_u8(self.ctx, rgb8.as_ptr(), 1, fn_ptr, depth.as_mut_ptr(), null_mut()) };
        unsafe { ffi::me_ctx_set_progress(self.ctx, None, null_mut()) };
        self.check(rc)?;
        Ok(depth)
    }
}

impl Drop for HipDevice {
    fn drop(&mut self) {
        unsafe { ffi::me_ctx_destroy(self.ctx) }
    }
}

fn last_error(ctx: *const ffi::MeCtx, code: i32) -> HipError {
    let message = unsafe { CStr::from_ptr(ffi::me_last_error(ctx)) }.to_string_lossy().into_owned();
    HipError { code, message }
}

/// output::DepthMap (output.rs:40-121) over the C ABI: `data` stays on the host like the reference's, the kernels
/// take it from there.
pub struct DepthMap<'d> {
    device: &'d HipDevice,
    pub data: Vec<f32>,
    pub data_width: usize,
    pub data_height: usize,
    pub original_size: (u32, u32),
    range: (f32, f32),
}

impl<'d> DepthMap<'d> {
    /// output.rs:44-75: clamp to [1/250, 1/0.1] + inverse_depth_range
    pub fn from_vec(device: &'d HipDevice, mut data: Vec<f32>, dims: [usize; 2], original_size: (u32, u32)) -> Result<Self, HipError> {
        let (mut mn, mut mx) = (0f32, 0f32);
        device.check(unsafe { ffi::me_depth_clamp_minmax(device.ctx, data.as_mut_ptr(), data.len() as i64, &mut mn, &mut mx) })?;
        Ok(DepthMap { device, data, data_width: dims[0], data_height: dims[1], original_size, range: (mn, mx) })
    }

    /// output.rs:123-131 output_depth_map before resize_exact + save (`depth_map_rgb_resized` includes the resize)
    pub fn depth_map_rgb(&self) -> Result<Vec<u8>, HipError> {
        let mut rgb = vec![0u8; self.data.len() * 3];
        self.device.check(unsafe {
            ffi::me_depthmap_rgb(self.device.ctx, self.data.as_ptr(), self.data.len() as i64, self.range.0, self.range.1, rgb.as_mut_ptr())
        })?;
        Ok(rgb)
    }

    /// output.rs:123-137 output_depth_map up to the save: the colour map and the resize to the original size, both on
    /// the GPU; the result is `RgbImage::from_raw(original_size.0, original_size.1, ..)`
    pub fn depth_map_rgb_resized(&self) -> Result<Vec<u8>, HipError> {
        let (ow, oh) = self.original_size;
        let mut rgb = vec![0u8; ow as usize * oh as usize * 3];
        self.device.check(unsafe {
            ffi::me_depthmap_rgb_resized(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32, self.range.0,
                                         self.range.1, null(), ow as i32, oh as i32, rgb.as_mut_ptr())
        })?;
        Ok(rgb)
    }

    /// output.rs:141-193 output_stereogram; `noise` is what :165-171 draws (one [u8; 3] per pixel, row by row)
    pub fn stereogram(&self, out_w: u32, out_h: u32, amplitude: f32, noise: &[u8]) -> Result<Vec<u8>, HipError> {
        assert_eq!(noise.len(), out_w as usize * out_h as usize * 3);
        let mut out = vec![0u8; noise.len()];
        self.device.check(unsafe {
            ffi::me_stereogram(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32, self.range.0,
                               self.range.1, out_w as i32, out_h as i32, amplitude, noise.as_ptr(), out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// output.rs:123-139 output_depth_map to a ".png" destination, whole: colour map, resize, row filters and deflate on
    /// the GPU; only the file's bytes come back
    pub fn output_depth_map_png(&self, destination_path: &str) -> Result<(), HipError> {
        let (ow, oh) = self.original_size;
        let dst = CString::new(destination_path).unwrap();
        self.device.check(unsafe {
            ffi::me_output_depth_map_png(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32, self.range.0,
                                         self.range.1, null(), ow as i32, oh as i32, dst.as_ptr())
        })
    }

    /// output.rs:141-193 output_stereogram to a ".png" destination, whole (`noise` as for `stereogram`)
    pub fn output_stereogram_png(&self, out_w: u32, out_h: u32, amplitude: f32, noise: &[u8], destination_path: &str) -> Result<(), HipError> {
        assert_eq!(noise.len(), out_w as usize * out_h as usize * 3);
        let dst = CString::new(destination_path).unwrap();
        self.device.check(unsafe {
            ffi::me_output_stereogram_png(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32, self.range.0,
                                          self.range.1, out_w as i32, out_h as i32, amplitude, noise.as_ptr(), dst.as_ptr())
        })
    }

    /// output.rs:123-139 output_depth_map to a ".jpg" / ".jpeg" destination, whole: colour map, resize and the baseline JPEG
    /// encoder on the GPU; only the file's bytes come back
    pub fn output_depth_map_jpeg(&self, quality: i32, subsampling: i32, destination_path: &str) -> Result<(), HipError> {
        let (ow, oh) = self.original_size;
        let dst = CString::new(destination_path).unwrap();
        self.device.check(unsafe {
            ffi::me_output_depth_map_jpeg(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32, self.range.0,
                                          self.range.1, null(), ow as i32, oh as i32, quality, subsampling, dst.as_ptr())
        })
    }

    /// output.rs:141-193 output_stereogram to a ".jpg" / ".jpeg" destination, whole (`noise` as for `stereogram`)
    pub fn output_stereogram_jpeg(&self, out_w: u32, out_h: u32, amplitude: f32, noise: &[u8], quality: i32, subsampling: i32,
                                  destination_path: &str) -> Result<(), HipError> {
        assert_eq!(noise.len(), out_w as usize * out_h as usize * 3);
        let dst = CString::new(destination_path).unwrap();
        self.device.check(unsafe {
            ffi::me_output_stereogram_jpeg(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32, self.range.0,
                                           self.range.1, out_w as i32, out_h as i32, amplitude, noise.as_ptr(), quality, subsampling,
                                           dst.as_ptr())
        })
    }

    /// output.rs:195-261 output_mesh with ObjWriter / PlyWriter (:385-630); vertex_mode = ME_VERTEX_*.  A ".glb"
    /// destination_path (any letter case) is written as a glTF 2.0 binary mesh; ".obj" and ".ply" as the reference does.
    pub fn output_mesh(&self, destination_path: &str, source_path: &str, vertex_mode: i32, vertex_colors: Option<&[u8]>) -> Result<(), HipError> {
        let dst = CString::new(destination_path).unwrap();
        let src = CString::new(source_path).unwrap();
        self.device.check(unsafe {
            ffi::me_output_mesh(self.device.ctx, self.data.as_ptr(), self.data_width as i32, self.data_height as i32,
                                self.original_size.0, self.original_size.1, dst.as_ptr(), src.as_ptr(), vertex_mode,
                                vertex_colors.map_or(null(), |c| c.as_ptr()))
        })
    }
}
