# Julia-side binding of libgsr_hip.so for GaussianSplatting.jl (reference @ v2.0.0).
#
# Could not be executed in the build environment (no Julia there); kept small and field-for-field
# identical to the ctypes binding that IS tested (gaussiansplatting.jl_amd/_lib.py + rasterizer.py).
#
# Design (what makes it a drop-in — every caller of the reference runs unchanged):
#   * callers keep holding the reference's own `GaussianRasterizer` — `Trainer{R <: GaussianRasterizer}`
#     (training.jl:185-194,225), the functor `rast(points, opacities, scales, rotations, f_dc, f_rest; ...)`
#     (rasterizer.jl:200-253, called at training.jl:646 / :501) and `rast.gstate.radii` / `rast.gstate.∇means_2d`
#     (strategy.jl:85-86) all keep working because nothing about that object changes;
#   * the native handle lives in a side table keyed by the rasterizer (`enable_hip_native!(rast)`); rasterizers
#     that were not enabled — e.g. the sky dome's second `GaussianRasterizer` (sky_dome.jl:144,191) unless it is
#     enabled too — fall through to the reference kernels via `invoke`;
#   * NO dispatch on keyword arguments (Julia has none): the two methods below are more specific than the
#     reference's only in their POSITIONAL types (ROCArray instead of AbstractArray), and branch on the side table;
#   * `rasterize` and `∇rasterize` are overridden; the reference's `ChainRulesCore.rrule` (rasterizer.jl:552-573) calls
#     exactly these two generics, so Zygote and the functor prologue are the reference's own code.  ONE rrule method is added
#     (same body as the reference's, ROCArray positional types): it tells the forward that a pullback will follow.  A
#     `rasterize` that is called directly — the reference's non-AD branch (rasterizer.jl:214-248): `validate`
#     (training.jl:501-504), the GUI (gui/worker.jl:654-657), scripts/render-views.jl — passes GSR_FORWARD_ONLY: same image,
#     no backward state written (a third of the forward's HBM traffic).  `enable_hip_native!(rast;
#     forward_only_outside_ad=false)` keeps the state for callers that run `∇rasterize` by hand after a bare `rasterize`;
#   * the library writes `radii` and `∇means_2d` straight into `rast.gstate` (gsr_aux.radii / gsr_grads.vmeans2d) and
#     the image into `rast.image`, so the reference's state object stays truthful.
#
# Replaces: src/rasterization/rasterizer.jl:255-408 (rasterize), :416-550 (∇rasterize).
module GaussianSplattingHipNative

using AMDGPU, StaticArrays
import KernelAbstractions as KA
import GPUArrays
import GaussianSplatting
import GaussianSplatting: GaussianRasterizer, GeometryState, Camera, resolution, n_color_features, rasterize, ∇rasterize
import ChainRulesCore
import ChainRulesCore: NoTangent, unthunk

const LIB = get(ENV, "GSR_HIP_LIB", "libgsr_hip.so")

struct GsrConfig
    width::Int32; height::Int32; mode::Int32
    near_plane::Float32; far_plane::Float32; radius_clip::Int32; blur_eps::Float32; flags::UInt32
    bins_budget_bytes::UInt64  # 0 = default
    ssim_precision::Int32      # per handle: 0 = process default (ssim_exact!), 1 fast, 2 exact            (ABI 6 encoding:
    preprocess_form::Int32     # per handle: 0 = process default (preprocess_form!), 1 direct, 2 aggregating   0 = default)
    form_tuner::Int32          # ABI 6: 0 default (on), 1 off, 2 on — the handle measures the binning form on 4K-class grids
    grad_precision::Int32      # ABI 6: 0 default, 1 the reference's arithmetic (accurate exp / division per pixel + its fp32 trees for
                               #        ∇scales / ∇rotations), 2 accurate exp / division + the float64 chain
end
struct GsrInputs
    n::Int32; n_coeffs::Int32; sh_degree::Int32
    means::Ptr{Float32}; shs::Ptr{Float32}; opacities::Ptr{Float32}
    scales::Ptr{Float32}; rotations::Ptr{Float32}
    background::NTuple{3, Float32}
end
struct GsrCamera
    R::NTuple{9, Float32}; t::NTuple{3, Float32}; focal::NTuple{2, Float32}
    principal::NTuple{2, Float32}; camera_center::NTuple{3, Float32}
    R_dev::Ptr{Float32}; t_dev::Ptr{Float32}
end
struct GsrAux; covisibilities::Ptr{UInt8}; uncertainties::Ptr{Float32}; radii::Ptr{Int32}; flags::UInt32; reserved::UInt32; end
const GSR_FLAG_ANTIALIASED = 0x00000004          # gsr_config.flags: opacity x add_blur's compensation, forward and backward
const GSR_BUF_COMPENSATIONS = Int32(10)          # gsr_buffer id: Float32 (N), the reference's `compensations` of the last forward
const GSR_FORWARD_ONLY = 0x00000001  # gsr_aux.flags: this forward will not be differentiated (no backward state kept)
struct GsrStats
    n_rendered::Int64; n_visible::Int32; max_tile_instances::Int32; generation::UInt64
    bins_bytes::Int64; compact_binning::Int32; preprocess_form::Int32
    # ABI 6: the handle's view history (include/gsr_policy.h), cumulative since gsr_create
    bins_regrowths::UInt32; compact_fallbacks::UInt32; tuner_rearms::UInt32; scratch_regrowths::UInt32
    fused_relaunches::UInt32; held_views::UInt32; bin_capacity::UInt32; tuner_form::Int32; tuner_ms::NTuple{2, Float32}
    tier_tiles::NTuple{3, UInt32}; reserved::UInt32
end
struct GsrGrads
    vmeans::Ptr{Float32}; vshs::Ptr{Float32}; vopacities::Ptr{Float32}
    vscales::Ptr{Float32}; vrotations::Ptr{Float32}; vR::Ptr{Float32}; vt::Ptr{Float32}
    vcolors::Ptr{Float32}          # C_NULL: classic form (∇shs written); see gsr.h for the factored multi-view form
    vmeans2d::Ptr{Float32}         # rast.gstate.∇means_2d
    forward_generation::UInt64     # pairs the pullback with its forward (0 = unchecked)
    flags::UInt32; reserved::UInt32 # GSR_GRADS_*
end
struct GsrTailState
    theta::NTuple{6, Ptr{Float32}}; mu::NTuple{6, Ptr{Float32}}; nu::NTuple{6, Ptr{Float32}}
    lr::NTuple{6, Float32}; current_step::NTuple{6, UInt32}
    beta1::Float32; beta2::Float32; eps::Float32; scale_dims::Int32
    shs::Ptr{Float32}; opacities_act::Ptr{Float32}; scales_act::Ptr{Float32}
    vmeans2d::Ptr{Float32}; forward_generation::UInt64
    flags::UInt32; reserved::UInt32
end
const EMPTY_STATS = GsrStats(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, (0f0, 0f0), (0x0, 0x0, 0x0), 0)
const GSR_GRADS_COLOR_COTANGENT = 0x00000001  # channels >= 4 of the cotangent (depth, alpha, normal) are zeros: ONLY valid for the
                                              # buffer loss_l1_ssim! wrote for this forward (the library checks pointer + generation)

check(rc) = rc == 0 || error(unsafe_string(ccall((:gsr_last_error_string, LIB), Cstring, ())))

# GSR_ABI_VERSION of the include/gsr.h these struct definitions mirror; checked (with the seven struct sizes) against
# the loaded library by the first enable_hip_native!: a stale libgsr_hip.so or a stale binding fails here, loudly.
const GSR_ABI_VERSION = 6
const ABI_CHECKED = Ref(false)
function check_abi()
    ABI_CHECKED[] && return
    check(ccall((:gsr_check_abi, LIB), Cint, (Cint, Csize_t, Csize_t, Csize_t, Csize_t, Csize_t, Csize_t, Csize_t), GSR_ABI_VERSION,
        sizeof(GsrConfig), sizeof(GsrInputs), sizeof(GsrCamera), sizeof(GsrAux), sizeof(GsrStats), sizeof(GsrGrads),
        sizeof(GsrTailState)))
    ABI_CHECKED[] = true
end
dptr(::Type{T}, x) where T = x === nothing ? Ptr{T}(C_NULL) : Ptr{T}(UInt(pointer(x)))
dptr(x) = dptr(Float32, x)
hipstream() = Ptr{Cvoid}(UInt(AMDGPU.stream().stream))  # the task-local stream (gui/worker.jl:47-51)

# ---- side table: reference rasterizer -> native handle ----
mutable struct NativeState
    handle::Ptr{Cvoid}
    generation::UInt64
    forward_only_outside_ad::Bool  # a bare `rasterize` (no rrule around it) keeps no backward state
    pullback_follows::Bool         # set by the rrule below for the forward it is about to run
    stats::GsrStats                # of the last forward (view history: `history(rast)`)
end
const NATIVE = WeakKeyDict{GaussianRasterizer, NativeState}()
const NATIVE_LOCK = ReentrantLock()
native(rast::GaussianRasterizer) = lock(() -> get(NATIVE, rast, nothing), NATIVE_LOCK)

"""
    enable_hip_native!(rast; reference_tile_lists=false, forward_only_outside_ad=true, ssim_exact=nothing, preprocess_form=nothing,
                       form_tuner=nothing, grad_precision=:default, antialiased=false)

Route `rasterize` / `∇rasterize` on this rasterizer through libgsr_hip.so.  Width / height / mode / near / far
are the rasterizer's own (rasterizer.jl:60-90).  `forward_only_outside_ad`: a `rasterize` that is not being
differentiated (no `rrule` around it) is rendered with GSR_FORWARD_ONLY — `∇rasterize` after it is an error.
`ssim_exact` (`nothing` | `false` | `true`) and `preprocess_form` (`nothing` | `0` | `1`) pin the two behaviour switches for THIS
rasterizer (ABI 5; constructor keywords, as the reference's knobs are: rasterizer.jl:60-65); `nothing` follows the process-wide
default (`ssim_exact!`, `preprocess_form!`) — so a GUI render task and a trainer in one process cannot disturb each other.
`form_tuner` (`nothing` | `false` | `true`): whether the handle measures the binning form on 4K-class grids (same outputs either
way).  `grad_precision` (`:default` | `:accurate` | `:fp32_reference`): the backward's arithmetic on needle-shaped splats —
`:accurate` = libm exp + IEEE division per pixel (+12 % of ∇render!; ∇means of a 90 : 1 needle 4e-4 -> 2e-5 from float64),
`:fp32_reference` = that and ∇scales / ∇rotations by the reference's own fp32 expression trees (projection.jl:132-257,
render.jl:302-366) instead of the library's float64 chain — for reference-parity runs.
`antialiased` (GSR_FLAG_ANTIALIASED): the Mip-Splatting 2-D filter the reference carries dormant — every opacity is multiplied by
`add_blur`'s compensation (render.jl:387-396) of the view, and `∇rasterize` returns the gradients of that image (∇opacities with
respect to the caller's opacity; ∇means / ∇scales / ∇rotations / the pose with `∇add_blur`, render.jl:398-413).  The factors of
the last forward are the handle's buffer `GSR_BUF_COMPENSATIONS`.
Returns `rast`.
"""
function enable_hip_native!(rast::GaussianRasterizer; reference_tile_lists::Bool = false, forward_only_outside_ad::Bool = true,
                            ssim_exact::Union{Nothing, Bool} = nothing, preprocess_form::Union{Nothing, Integer} = nothing,
                            form_tuner::Union{Nothing, Bool} = nothing, grad_precision::Symbol = :default,
                            antialiased::Bool = false)
    native(rast) === nothing || return rast
    check_abi()
    c, w, h = size(rast.image)
    href = Ref{Ptr{Cvoid}}()
    check(ccall((:gsr_create, LIB), Cint, (Ref{GsrConfig}, Ref{Ptr{Cvoid}}),
        GsrConfig(w, h, c, rast.near_plane, rast.far_plane, 3, 0.3f0,
                  UInt32(reference_tile_lists ? 0x2 : 0x0) | (antialiased ? GSR_FLAG_ANTIALIASED : 0x00000000), 0,
                  # ABI 6: 0 = default, 1 / 2 the explicit choices
                  ssim_exact === nothing ? Int32(0) : Int32(ssim_exact ? 2 : 1),
                  preprocess_form === nothing ? Int32(0) : Int32(preprocess_form != 0 ? 2 : 1),
                  form_tuner === nothing ? Int32(0) : Int32(form_tuner ? 2 : 1),
                  Int32(grad_precision === :fp32_reference ? 1 : grad_precision === :accurate ? 2 : 0)),
        href))
    st = NativeState(href[], 0, forward_only_outside_ad, false, EMPTY_STATS)
    finalizer(s -> ccall((:gsr_destroy, LIB), Cint, (Ptr{Cvoid},), s.handle), st)
    lock(() -> (NATIVE[rast] = st), NATIVE_LOCK)
    return rast
end

"""
    loss_l1_ssim!(rast, target; λ_dssim=0.2f0) -> (loss::ROCVector{Float32} of length 1, vpixels)

The photometric loss head of `step!` (training.jl:656,684-694) fused with its pullback (gsr_loss_l1_ssim) on `rast.image`, the render
of the forward just run: `target` is the (W,H,3) device image.  The returned cotangent has exact zeros above the colour channels and
is the ONLY buffer `backward_trainer_tail!(...; color_cotangent=true)` accepts — the library remembers which buffer its loss head
wrote for which forward, so a cotangent with depth / normal terms can never be mistaken for it (ADVICE r5: the flag used to be a
sticky, unchecked promise).
"""
function loss_l1_ssim!(rast::GaussianRasterizer, target; λ_dssim::Float32 = 0.2f0)
    st = native(rast)
    st === nothing && error("loss_l1_ssim! needs enable_hip_native!(rast)")
    loss = AMDGPU.zeros(Float32, 1); vpixels = similar(rast.image)
    check(ccall((:gsr_loss_l1_ssim, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
        st.handle, dptr(rast.image), dptr(target), λ_dssim, dptr(loss), dptr(vpixels), hipstream()))
    return loss, vpixels
end

"""
    history(rast) -> NamedTuple

The native handle's view history after the last forward (gsr_stats, ABI 6): how often the key bins were regrown, a view fell back
to compact binning, the form tuner started over, a scratch buffer was reallocated — in a steady training run none of them moves.
"""
function history(rast::GaussianRasterizer)
    s = native(rast).stats
    return (; s.bins_regrowths, s.compact_fallbacks, s.tuner_rearms, s.scratch_regrowths, s.fused_relaunches, s.held_views,
            s.bin_capacity, s.tuner_form, s.compact_binning, s.preprocess_form)
end

function disable_hip_native!(rast::GaussianRasterizer)
    lock(() -> delete!(NATIVE, rast), NATIVE_LOCK)  # the finalizer of the NativeState destroys the handle
    return rast
end

function _structs(means_3d, shs, opacities, scales, rotations, R_w2c, t_w2c, camera::Camera, sh_degree, background)
    K = camera.intrinsics
    R = SMatrix{3, 3, Float32}(camera.w2c[1:3, 1:3]); t = SVector{3, Float32}(camera.w2c[1:3, 4])
    inp = GsrInputs(size(means_3d, 2), size(shs, 2), sh_degree, dptr(means_3d), dptr(shs), dptr(opacities),
        dptr(scales), dptr(rotations), Tuple(background))
    cam = GsrCamera(Tuple(R), Tuple(t), Tuple(K.focal), Tuple(K.principal), Tuple(camera.camera_center),
        dptr(R_w2c), dptr(t_w2c))
    return inp, cam
end

const RM = ROCMatrix{Float32}
const R3 = ROCArray{Float32, 3}
const REF_FWD_SIG = Tuple{AbstractMatrix{Float32}, AbstractArray{Float32, 3}, AbstractMatrix{Float32},
                          AbstractMatrix{Float32}, AbstractMatrix{Float32}, Any, Any}
const REF_BWD_SIG = Tuple{AbstractArray{Float32, 3}, AbstractMatrix{Float32}, AbstractArray{Float32, 3},
                          AbstractMatrix{Float32}, AbstractMatrix{Float32}, AbstractMatrix{Float32},
                          AbstractVector{Int32}, Any, Any}

# rasterize(means_3d, shs, opacities, scales, rotations, R_w2c, t_w2c; rast, camera, ...) — rasterizer.jl:255-408
function GaussianSplatting.rasterize(means_3d::RM, shs::R3, opacities::RM, scales::RM, rotations::RM,
        R_w2c = nothing, t_w2c = nothing;
        rast::GaussianRasterizer, camera::Camera, sh_degree::Int, background::SVector{3, Float32},
        covisibilities = nothing, uncertainties = nothing)
    st = native(rast)
    st === nothing && return invoke(rasterize, REF_FWD_SIG, means_3d, shs, opacities, scales, rotations, R_w2c, t_w2c;
        rast, camera, sh_degree, background, covisibilities, uncertainties)
    n = size(means_3d, 2)
    if length(rast.gstate) < n  # rasterizer.jl:275-278: the reference's own grow-only GeometryState
        KA.unsafe_free!(rast.gstate)
        rast.gstate = GPUArrays.@uncached GeometryState(KA.get_backend(rast), n; n_features=n_color_features(rast.mode))
    end
    inp, cam = _structs(means_3d, shs, opacities, scales, rotations, R_w2c, t_w2c, camera, sh_degree, background)
    keep = st.pullback_follows || !st.forward_only_outside_ad
    st.pullback_follows = false
    aux = GsrAux(dptr(UInt8, covisibilities), dptr(uncertainties), dptr(Int32, rast.gstate.radii),
        keep ? 0x00000000 : GSR_FORWARD_ONLY, 0x00000000)
    stats = Ref(EMPTY_STATS)
    check(ccall((:gsr_forward, LIB), Cint,
        (Ptr{Cvoid}, Ref{GsrInputs}, Ref{GsrCamera}, Ptr{Float32}, Ref{GsrAux}, Ptr{Cvoid}, Ref{GsrStats}),
        st.handle, inp, cam, dptr(rast.image), aux, hipstream(), stats))
    st.generation = stats[].generation
    st.stats = stats[]
    return rast.image  # aliased, overwritten by the next call (rasterizer.jl:407)
end

# ∇rasterize(vpixels, means_3d, shs, scales, rotations, opacities, radii, R_w2c, t_w2c; rast, ...) — rasterizer.jl:416-550
# (called by the reference's rrule pullback, rasterizer.jl:565-570, with radii = rast.gstate.radii)
function GaussianSplatting.∇rasterize(vpixels::R3, means_3d::RM, shs::R3, scales::RM, rotations::RM, opacities::RM,
        radii::ROCVector{Int32}, R_w2c = nothing, t_w2c = nothing;
        rast::GaussianRasterizer, camera::Camera, sh_degree::Int, background::SVector{3, Float32})
    st = native(rast)
    st === nothing && return invoke(∇rasterize, REF_BWD_SIG, vpixels, means_3d, shs, scales, rotations, opacities,
        radii, R_w2c, t_w2c; rast, camera, sh_degree, background)
    # fresh gradient arrays per call, as the reference (rasterizer.jl:437-445); the library overwrites every element
    vmeans = similar(means_3d); vshs = similar(shs); vopac = similar(opacities)
    vscales = similar(scales); vrot = similar(rotations)
    vR = R_w2c === nothing ? nothing : AMDGPU.zeros(Float32, 3, 3)
    vt = R_w2c === nothing ? nothing : AMDGPU.zeros(Float32, 3)
    inp, cam = _structs(means_3d, shs, opacities, scales, rotations, R_w2c, t_w2c, camera, sh_degree, background)
    g = GsrGrads(dptr(vmeans), dptr(vshs), dptr(vopac), dptr(vscales), dptr(vrot), dptr(vR), dptr(vt),
        Ptr{Float32}(C_NULL), Ptr{Float32}(UInt(pointer(rast.gstate.∇means_2d))), st.generation,
        # (no GSR_GRADS_COLOR_COTANGENT here: under the rrule the cotangent is Zygote's, not the fused loss head's)
        UInt32(0), UInt32(0))
    check(ccall((:gsr_backward, LIB), Cint,
        (Ptr{Cvoid}, Ref{GsrInputs}, Ref{GsrCamera}, Ptr{Float32}, Ref{GsrGrads}, Ptr{Cvoid}),
        st.handle, inp, cam, dptr(vpixels), g, hipstream()))
    return vmeans, vshs, vopac, vscales, vrot, vR, vt
end

# The pullback hands over `unthunk(vpixels)` (rasterizer.jl:567): under Zygote that can be a `FillArrays.Fill`, a
# `Base.ReshapedArray` or a CPU array instead of a ROCArray.  Without this method dispatch would quietly fall through to the
# reference's kernels for an ENABLED rasterizer (correct, but an invisible performance cliff — and on a forward that kept its
# state in the library, not in rast.bstate, a wrong one).  Materialise the cotangent once and say so.
function GaussianSplatting.∇rasterize(vpixels::AbstractArray{Float32, 3}, means_3d::RM, shs::R3, scales::RM, rotations::RM,
        opacities::RM, radii::ROCVector{Int32}, R_w2c = nothing, t_w2c = nothing;
        rast::GaussianRasterizer, camera::Camera, sh_degree::Int, background::SVector{3, Float32})
    native(rast) === nothing && return invoke(∇rasterize, REF_BWD_SIG, vpixels, means_3d, shs, scales, rotations, opacities,
        radii, R_w2c, t_w2c; rast, camera, sh_degree, background)
    @warn "GaussianSplattingHipNative: cotangent of type $(typeof(vpixels)) copied into a ROCArray for the native ∇rasterize" maxlog=1
    vp = similar(rast.image)
    vp .= vpixels
    return ∇rasterize(vp, means_3d, shs, scales, rotations, opacities, radii, R_w2c, t_w2c; rast, camera, sh_degree, background)
end

# rrule(rasterize, ...) — the reference's own (rasterizer.jl:552-573) with ROCArray positional types: the only addition is the
# note to the forward that this render WILL be differentiated (a bare `rasterize` is rendered forward-only).
function ChainRulesCore.rrule(::typeof(rasterize), means_3d::RM, shs::R3, opacities::RM, scales::RM, rotations::RM,
        R_w2c = nothing, t_w2c = nothing;
        rast::GaussianRasterizer, camera::Camera, sh_degree::Int, background::SVector{3, Float32},
        covisibilities = nothing, uncertainties = nothing)
    st = native(rast)
    st === nothing || (st.pullback_follows = true)
    image = rasterize(means_3d, shs, opacities, scales, rotations, R_w2c, t_w2c;
        rast, camera, sh_degree, background, covisibilities, uncertainties)
    function _pullback(vpixels)
        ∇ = ∇rasterize(unthunk(vpixels), means_3d, shs, scales, rotations, opacities,
            rast.gstate.radii, R_w2c, t_w2c; rast, camera, sh_degree, background)
        return (NoTangent(), ∇...)
    end
    return image, _pullback
end

# gsr_reserve: pre-size the native scratch for up to n_gaussians / n_instances (call it after a densification round, with headroom:
# a reallocation inside a forward synchronises the device in the middle of a training step).  `rast.gstate` — whose radii /
# ∇means_2d arrays the native forward / backward write through gsr_aux.radii / gsr_grads.vmeans2d — is pre-sized with it.
# A reserve that REPLACES anything ends the live forward (include/gsr.h: gsr_reserve): the library does when it reallocates a
# buffer that existed; when only `rast.gstate` is replaced here, the handle still holds the old radii array's address from the
# last forward, so it is told (gsr_drop_forward) BEFORE that array is freed.  Until the next `rasterize`, ∇rasterize /
# backward_trainer_tail! / update_stats! then fail with GSR_E_STATE instead of reading freed memory: reserve after update_stats!.
function reserve!(rast::GaussianRasterizer, n_gaussians::Integer, n_instances::Integer = 0)
    st = native(rast)
    st === nothing && return rast
    check(ccall((:gsr_reserve, LIB), Cint, (Ptr{Cvoid}, Int64, Int64), st.handle, n_gaussians, n_instances))
    if length(rast.gstate) < n_gaussians
        check(ccall((:gsr_drop_forward, LIB), Cint, (Ptr{Cvoid},), st.handle))
        KA.unsafe_free!(rast.gstate)
        rast.gstate = GPUArrays.@uncached GeometryState(KA.get_backend(rast), Int(n_gaussians); n_features=n_color_features(rast.mode))
    end
    return rast
end

# release_scene_buffers!(rast) (rasterizer.jl:111-123) also has to drop the library's scene-sized scratch
function release_native_scene_buffers!(rast::GaussianRasterizer)
    st = native(rast)
    st === nothing || check(ccall((:gsr_release_scene_buffers, LIB), Cint, (Ptr{Cvoid},), st.handle))
    return
end

# ---- process-wide switches ----

# Form of the binning inside the forward's first kernel: -1 by scene and grid size (default), 0 direct, 1 aggregating wherever
# its LDS fits.  Identical outputs in every form (include/gsr.h: gsr_preprocess_form); a performance switch.
preprocess_form!(form::Integer) = check(ccall((:gsr_preprocess_form, LIB), Cint, (Cint,), form))
# Arithmetic of the SSIM entry points: false = contracted (default), true = every fp32 operation as written (gsr_ssim_precision)
ssim_exact!(exact::Bool) = check(ccall((:gsr_ssim_precision, LIB), Cint, (Cint,), exact ? 1 : 0))

# Optional (not a reference function): 63-bit Morton codes of the positions (3 x N Float32 device array) inside the box
# lo .. hi — sortperm of them is the permutation of a spatial re-sort (apply it to every per-Gaussian array, `gs.ids` included).
function morton_codes!(codes, points, lo::NTuple{3,Float32}, hi::NTuple{3,Float32})
    n = size(points, 2)
    check(ccall((:gsr_morton_codes, LIB), Cint, (Int64, Ptr{Float32}, Ref{NTuple{3,Float32}}, Ref{NTuple{3,Float32}}, Ptr{UInt64}, Ptr{Cvoid}),
                n, dptr(points), Ref(lo), Ref(hi), dptr(UInt64, codes), hipstream()))
    return codes
end

# compute_scales (dataset.jl:236-249) on the device: the exact three nearest neighbours of every point of `points`
# (3 x N Float32 device array) and the reference's scale from them, written to `scales` (3 x N, or 1 x N for an isotropic
# model).  `order`: a device Int32 vector of N 0-based row numbers that groups the search (sortperm of morton_codes! .- 1),
# or nothing; the result does not depend on it.  `dist2` (3 x N), when given, receives the squared distances, ascending.
knn_scratch_bytes(n::Integer) = Int(ccall((:gsr_knn_scratch_bytes, LIB), Csize_t, (Int64,), n))
function knn_scales!(scales, points; order = nothing, point_size::Float32 = 1f0, dist2 = nothing, scratch = nothing)
    n = size(points, 2)
    nb = knn_scratch_bytes(n)
    scratch === nothing && (scratch = AMDGPU.zeros(UInt8, nb))
    check(ccall((:gsr_knn_scales, LIB), Cint,
        (Int64, Ptr{Float32}, Ptr{Int32}, Float32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        n, dptr(points), dptr(Int32, order), point_size, size(scales, 1), dptr(scales), dptr(dist2), dptr(Cvoid, scratch), nb,
        hipstream()))
    return scales
end

# ---- optional fused tails (not needed for the drop-in; callers opt in) ----

# update_stats!(strategy, radii, ∇means_2d, resolution) (strategy.jl:107-136) on the library's kernel
update_stats!(strategy, rast::GaussianRasterizer) = check(ccall((:gsr_update_stats, LIB), Cint,
    (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}), native(rast).handle,
    dptr(Int32, strategy.max_radii), dptr(strategy.accum_∇means_2d), dptr(strategy.denom), hipstream()))

# The tail of `step!` (training.jl:768-779 + the prologue of the next `rast(...)` call, rasterizer.jl:218-247) in one
# pass: `∇` are the cotangents ∇rasterize returned (w.r.t. the ACTIVATED opacity / scale), `θ` the raw parameter
# arrays and `opts` the six NU.Adam in OPTIMIZER_NAMES order; shs / opacities_act / scales_act are the activated
# copies of this step on entry and of the updated parameters on exit.
struct GsrTailGrads; vmeans::Ptr{Float32}; vshs::Ptr{Float32}; vopacities::Ptr{Float32}; vscales::Ptr{Float32}; vrotations::Ptr{Float32}; end
function trainer_tail_step!(θ::NTuple{6}, opts::NTuple{6}, ∇, shs, opacities_act, scales_act; β1=0.9f0, β2=0.999f0, ϵ=1f-15)
    vmeans, vshs, vopac, vscales, vrot = ∇
    p(xs) = Ptr{Float32}[dptr(x) for x in xs]
    steps = UInt32[o.current_step + 0x1 for o in opts]  # the counters AFTER their increment, committed below
    check(ccall((:gsr_trainer_tail_step, LIB), Cint,
        (Cint, Cint, Cint, Ref{GsrTailGrads}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Ptr{Cfloat}, Ptr{UInt32},
         Cfloat, Cfloat, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
        size(θ[1], 2), size(θ[3], 2), size(θ[5], 1), GsrTailGrads(dptr(vmeans), dptr(vshs), dptr(vopac), dptr(vscales), dptr(vrot)),
        p(θ), p(map(o -> o.μ[1], opts)), p(map(o -> o.ν[1], opts)), Float32[o.lr for o in opts],
        steps, β1, β2, ϵ, dptr(shs), dptr(opacities_act), dptr(scales_act), hipstream()))
    foreach(o -> o.current_step += 0x1, opts)
end

# The same tail applied in the epilogue of the backward (gsr_backward_trainer_tail): the single-GPU `step!` after
# the loss with no gradient arrays at all.  `vpixels` is the loss cotangent of rast.image; θ[1] / θ[6] must be the
# arrays the forward was given as means_3d / rotations, shs / opacities_act / scales_act its other inputs.
# `color_cotangent = true` (per call, GSR_GRADS_COLOR_COTANGENT): `vpixels` is the buffer loss_l1_ssim! returned for this forward,
# untouched — in :rgbd / :rgbdn mode the backward then runs the :rgb arithmetic (:rgbdn 0.885 -> 0.702 ms at config 3); any other
# buffer with the flag set is an error, not silently dropped depth / normal gradients.
function backward_trainer_tail!(rast::GaussianRasterizer, vpixels, θ::NTuple{6}, opts::NTuple{6}, shs, opacities_act,
        scales_act; camera::Camera, sh_degree::Int, background::SVector{3, Float32}, β1=0.9f0, β2=0.999f0, ϵ=1f-15,
        color_cotangent::Bool = false)
    st = native(rast)
    st === nothing && error("backward_trainer_tail! needs enable_hip_native!(rast)")
    inp, cam = _structs(θ[1], shs, opacities_act, scales_act, θ[6], nothing, nothing, camera, sh_degree, background)
    p(xs) = ntuple(i -> dptr(xs[i]), 6)
    ts = GsrTailState(p(θ), p(map(o -> o.μ[1], opts)), p(map(o -> o.ν[1], opts)), ntuple(i -> Float32(opts[i].lr), 6),
        ntuple(i -> UInt32(opts[i].current_step + 0x1), 6), β1, β2, ϵ, size(θ[5], 1),
        dptr(shs), dptr(opacities_act), dptr(scales_act), Ptr{Float32}(UInt(pointer(rast.gstate.∇means_2d))), st.generation,
        color_cotangent ? GSR_GRADS_COLOR_COTANGENT : UInt32(0), UInt32(0))
    check(ccall((:gsr_backward_trainer_tail, LIB), Cint,
        (Ptr{Cvoid}, Ref{GsrInputs}, Ref{GsrCamera}, Ptr{Float32}, Ref{GsrTailState}, Ptr{Cvoid}),
        st.handle, inp, cam, dptr(vpixels), ts, hipstream()))
    foreach(o -> o.current_step += 0x1, opts)
end

# ---- bilateral grid (src/bilateral_grid.jl) ----

# bilateral_slice(image, grid) (bilateral_grid.jl:75-85) on gsr_bilateral_slice_forward: a method for device arrays, so
# `step!` (training.jl:679-681) reaches it unchanged.  Channels >= 3 of a (C,W,H) image are copied.
function GaussianSplatting.bilateral_slice(image::ROCArray{Float32, 3}, grid::ROCArray{Float32, 4})
    out = similar(image)
    check(ccall((:gsr_bilateral_slice_forward, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Int32, Int32, Int32, Ptr{Float32}, Ptr{Cvoid}),
        size(image, 2), size(image, 3), size(image, 1), dptr(image), dptr(grid), size(grid, 1), size(grid, 2), size(grid, 3),
        dptr(out), hipstream()))
    return out
end

# its rrule (bilateral_grid.jl:87-100) on gsr_bilateral_slice_backward: no float atomics, run-to-run bit-identical ∇grid
function ChainRulesCore.rrule(::typeof(GaussianSplatting.bilateral_slice), image::ROCArray{Float32, 3},
        grid::ROCArray{Float32, 4})
    out = GaussianSplatting.bilateral_slice(image, grid)
    function _bilateral_slice_pullback(Δ)
        vout = ROCArray{Float32}(unthunk(Δ))
        ∇image = similar(image); ∇grid = similar(grid)
        w, h, gx, gy, gz = size(image, 2), size(image, 3), size(grid, 1), size(grid, 2), size(grid, 3)
        nb = ccall((:gsr_bilateral_scratch_bytes, LIB), Csize_t, (Int32, Int32, Int32, Int32, Int32), w, h, gx, gy, gz)
        scratch = AMDGPU.zeros(UInt8, max(Int(nb), 1))
        check(ccall((:gsr_bilateral_slice_backward, LIB), Cint,
            (Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
             Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
            w, h, size(image, 1), dptr(image), dptr(grid), gx, gy, gz, dptr(vout), dptr(∇image), dptr(∇grid),
            Ptr{Cvoid}(UInt(pointer(scratch))), Csize_t(length(scratch)), hipstream()))
        return NoTangent(), ∇image, ∇grid
    end
    return out, _bilateral_slice_pullback
end

# Optional (callers opt in): `NU.step!(bgrid.optimizer, bgrid.grids, ∇grids)` (training.jl:784-790) with ∇grids =
# tv_weight·∇tv_loss + the view's slice gradient `∇grid_view`, in one pass (gsr_bilateral_adam_tail); returns the device
# scalar tv_weight·tv_loss of the grids before the update (the `tv_term` of training.jl:704-705).  `view` is 1-based.
function bilateral_adam_tail!(bgrid, ∇grid_view, view::Integer; tv_weight::Float32 = 10f0, β1=0.9f0, β2=0.999f0, ϵ=1f-15)
    grids, opt = bgrid.grids, bgrid.optimizer
    gx, gy, gz, _, n = size(grids)
    tv = AMDGPU.zeros(Float32, 1)
    nb = ccall((:gsr_bilateral_tv_scratch_bytes, LIB), Csize_t, (Int32,), n)
    scratch = AMDGPU.zeros(UInt8, max(Int(nb), 1))
    check(ccall((:gsr_bilateral_adam_tail, LIB), Cint,
        (Int32, Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, Cfloat, Cfloat, UInt32,
         Cfloat, Cfloat, Cfloat, Ptr{Float32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        n, gx, gy, gz, dptr(grids), dptr(opt.μ[1]), dptr(opt.ν[1]), dptr(∇grid_view), view - 1, tv_weight, Float32(opt.lr),
        UInt32(opt.current_step + 0x1), β1, β2, ϵ, dptr(tv), Ptr{Cvoid}(UInt(pointer(scratch))), Csize_t(length(scratch)),
        hipstream()))
    opt.current_step += 0x1
    return tv
end

# ---- geometry regularisation (src/geometry_regularization.jl; `use_normal_loss`, training.jl:625-733) ----

# the kernels read focal and principal only (the rays of `pixel_rays`)
function _camera_only(camera::Camera)
    K = camera.intrinsics
    R = SMatrix{3, 3, Float32}(camera.w2c[1:3, 1:3]); t = SVector{3, Float32}(camera.w2c[1:3, 4])
    return GsrCamera(Tuple(R), Tuple(t), Tuple(K.focal), Tuple(K.principal), Tuple(camera.camera_center),
        dptr(nothing), dptr(nothing))
end

function _normal_loss_scratch(w, h)
    nb = ccall((:gsr_normal_loss_scratch_bytes, LIB), Csize_t, (Int32, Int32), w, h)
    return AMDGPU.zeros(UInt8, max(Int(nb), 4))
end

# weight · depth_normal_consistency_loss (geometry_regularization.jl:87-183) of the (8,W,H) :rgbdn frame `image`
# (channel 4 = blended depth, 5 = alpha, 6:8 = the blended normal, 1-based) on gsr_normal_loss_forward: a device scalar;
# the rays are computed in the kernel from `camera`, the "too little evidence" gate is applied on the device.
# Returns (loss, scratch): `scratch` is what depth_normal_loss_backward! of the same image reads.
function depth_normal_loss(image::ROCArray{Float32, 3}, camera::Camera; weight::Float32 = 0.05f0,
        scratch = _normal_loss_scratch(size(image, 2), size(image, 3)))
    loss = AMDGPU.zeros(Float32, 1); stats = AMDGPU.zeros(Float32, 2)
    check(ccall((:gsr_normal_loss_forward, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ref{GsrCamera}, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid},
         Csize_t, Ptr{Cvoid}),
        size(image, 2), size(image, 3), size(image, 1), dptr(image), _camera_only(camera), weight, dptr(loss), dptr(stats),
        dptr(nothing), Ptr{Cvoid}(UInt(pointer(scratch))), Csize_t(length(scratch)), hipstream()))
    return loss, scratch
end

# ADDS weight · ∂loss/∂(depth, alpha, normal) onto channels 4:8 of `vpixels` (8,W,H) in place (gsr_normal_loss_backward):
# no float atomics, run-to-run bit-identical.  A `vpixels` this was added onto must go to the backward WITHOUT
# `color_cotangent = true`.
function depth_normal_loss_backward!(vpixels::ROCArray{Float32, 3}, image::ROCArray{Float32, 3}, camera::Camera, scratch;
        weight::Float32 = 0.05f0)
    size(vpixels) == size(image) || error("vpixels must have the image's size")
    check(ccall((:gsr_normal_loss_backward, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ref{GsrCamera}, Cfloat, Ptr{Float32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        size(image, 2), size(image, 3), size(image, 1), dptr(image), _camera_only(camera), weight, dptr(vpixels),
        Ptr{Cvoid}(UInt(pointer(scratch))), Csize_t(length(scratch)), hipstream()))
    return vpixels
end

function ChainRulesCore.rrule(::typeof(depth_normal_loss), image::ROCArray{Float32, 3}, camera::Camera;
        weight::Float32 = 0.05f0)
    loss, scratch = depth_normal_loss(image, camera; weight)
    function _depth_normal_loss_pullback(Δ)
        ∇image = AMDGPU.zeros(Float32, size(image))
        depth_normal_loss_backward!(∇image, image, camera, scratch; weight)
        δ = unthunk(Δ)[1]
        return NoTangent(), ∇image .* δ, NoTangent()
    end
    return (loss, scratch), _depth_normal_loss_pullback
end

# weight · flatten_loss(scales) (geometry_regularization.jl:197-211) over the raw (3,N) / (1,N) scales as a device
# scalar (gsr_flatten_loss); with `vscales` (3,N) — the ∇scales gsr_backward wrote, w.r.t. the ACTIVATED scale — the
# constant weight / N is added onto it on each Gaussian's first minimal axis.  The fused backward_trainer_tail! has no
# gradient arrays: steps with the regulariser on run ∇rasterize + flatten_loss!(...; vscales) + trainer_tail_step!.
function flatten_loss!(scales::ROCArray{Float32, 2}; weight::Float32 = 0.005f0, vscales = nothing)
    n = size(scales, 2)
    loss = AMDGPU.zeros(Float32, 1)
    nb = ccall((:gsr_flatten_loss_scratch_bytes, LIB), Csize_t, (Int32,), n)
    scratch = AMDGPU.zeros(UInt8, max(Int(nb), 4))
    check(ccall((:gsr_flatten_loss, LIB), Cint,
        (Int32, Int32, Ptr{Float32}, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        n, size(scales, 1), dptr(scales), weight, dptr(loss), dptr(vscales), Ptr{Cvoid}(UInt(pointer(scratch))),
        Csize_t(length(scratch)), hipstream()))
    return loss
end

function ChainRulesCore.rrule(::typeof(flatten_loss!), scales::ROCArray{Float32, 2}; weight::Float32 = 0.005f0)
    loss = flatten_loss!(scales; weight)
    function _flatten_loss_pullback(Δ)
        v = AMDGPU.zeros(Float32, 3, size(scales, 2))
        flatten_loss!(scales; weight, vscales = v)
        δ = unthunk(Δ)[1]
        return NoTangent(), v[1:size(scales, 1), :] .* exp.(scales) .* δ   # the prologue's pullback: ∂exp(s)/∂s
    end
    return loss, _flatten_loss_pullback
end

# ---- anchored depth supervision (src/depth_supervision.jl:406-536; `use_depth_loss`, training.jl:604-620,709-718) ----

# gsr_depth_anchor: the fields of the reference's DepthAnchor, in its order
struct GsrDepthAnchor; a::Float32; b::Float32; floor::Float32; disparity::Float32; p_far::Float32; end
GsrDepthAnchor(anchor) = GsrDepthAnchor(anchor.a, anchor.b, anchor.floor, anchor.disparity, anchor.p_far)

function _depth_loss_scratch(w, h)
    nb = ccall((:gsr_depth_loss_scratch_bytes, LIB), Csize_t, (Int32, Int32), w, h)
    return AMDGPU.zeros(UInt8, max(Int(nb), 16))
end

# `depth_target` on the device: (target, half_band, flags) of the (W,H) prior; flags: bit 0 valid, bit 1 far_extrap
function depth_target(anchor, prior::ROCArray{Float32, 2}, qstep::Float32)
    target = similar(prior); half_band = similar(prior); flags = AMDGPU.zeros(UInt8, size(prior))
    check(ccall((:gsr_depth_target, LIB), Cint,
        (Int32, Int32, Ptr{Float32}, Ref{GsrDepthAnchor}, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
        size(prior, 1), size(prior, 2), dptr(prior), GsrDepthAnchor(anchor), qstep, dptr(target), dptr(half_band),
        Ptr{UInt8}(UInt(pointer(flags))), hipstream()))
    return target, half_band, flags
end

# weight · ssi_depth_loss of the (C,W,H) frame `image` (C = 5 or 8; channel 4 = blended depth, 5 = alpha, 1-based) against
# the target built in the kernel from `prior` (W,H) and `anchor`: a device scalar (gsr_depth_loss_forward).
# Returns (loss, scratch): `scratch` is what depth_loss_backward! of the same image reads.
function depth_loss(image::ROCArray{Float32, 3}, prior::ROCArray{Float32, 2}, anchor, qstep::Float32; weight::Float32,
        λ_grad::Float32 = 1f0, scratch = _depth_loss_scratch(size(image, 2), size(image, 3)))
    loss = AMDGPU.zeros(Float32, 1); stats = AMDGPU.zeros(Float32, 4)
    check(ccall((:gsr_depth_loss_forward, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ref{GsrDepthAnchor}, Cfloat, Cfloat, Cfloat, Ptr{Float32},
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        size(image, 2), size(image, 3), size(image, 1), dptr(image), dptr(prior), GsrDepthAnchor(anchor), qstep, λ_grad,
        weight, dptr(loss), dptr(stats), dptr(nothing), dptr(nothing), Ptr{UInt8}(0), Ptr{Cvoid}(UInt(pointer(scratch))),
        Csize_t(length(scratch)), hipstream()))
    return loss, scratch
end

# ADDS weight · ∂ssi_depth_loss/∂(depth, alpha) onto channels 4:5 of `vpixels` (C,W,H) in place (gsr_depth_loss_backward):
# no float atomics, run-to-run bit-identical.  A `vpixels` this was added onto must go to the backward WITHOUT
# `color_cotangent = true`.
function depth_loss_backward!(vpixels::ROCArray{Float32, 3}, image::ROCArray{Float32, 3}, prior::ROCArray{Float32, 2},
        anchor, qstep::Float32, scratch; weight::Float32, λ_grad::Float32 = 1f0)
    size(vpixels) == size(image) || error("vpixels must have the image's size")
    check(ccall((:gsr_depth_loss_backward, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ref{GsrDepthAnchor}, Cfloat, Cfloat, Cfloat, Ptr{Float32},
         Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        size(image, 2), size(image, 3), size(image, 1), dptr(image), dptr(prior), GsrDepthAnchor(anchor), qstep, λ_grad,
        weight, dptr(vpixels), Ptr{Cvoid}(UInt(pointer(scratch))), Csize_t(length(scratch)), hipstream()))
    return vpixels
end

function ChainRulesCore.rrule(::typeof(depth_loss), image::ROCArray{Float32, 3}, prior::ROCArray{Float32, 2}, anchor,
        qstep::Float32; weight::Float32, λ_grad::Float32 = 1f0)
    loss, scratch = depth_loss(image, prior, anchor, qstep; weight, λ_grad)
    function _depth_loss_pullback(Δ)
        ∇image = AMDGPU.zeros(Float32, size(image))
        depth_loss_backward!(∇image, image, prior, anchor, qstep, scratch; weight, λ_grad)
        δ = unthunk(Δ)[1]
        return NoTangent(), ∇image .* δ, NoTangent(), NoTangent(), NoTangent()
    end
    return (loss, scratch), _depth_loss_pullback
end

# weight · final_scale^clamp(step / steps, 0, 1): the decay of the term's weight over training
depth_weight(step; weight::Float32 = 2f0, final_scale::Float32 = 0.02f0, steps = 30_000) =
    weight * final_scale^clamp(Float32(step) / Float32(steps), 0f0, 1f0)

# ---- MCMCStrategy on the device (src/mcmc.jl; include/gsr.h: gsr_mcmc_*) ----
# The reference's relocate_gaussians! / add_gaussians! / split_sampled! / multinomial_sample are chains of device->host
# copies, host loops and re-uploads (mcmc.jl:135-258); here every per-Gaussian pass is one launch.  Two intended deviations
# (include/gsr.h): random numbers come from the library's counter-based generator (the caller passes a fresh `seed` per draw
# / step), and the multinomial draw runs on integer weights floor(sigmoid(o)·2^30) with exact UInt64 prefix sums.  Row
# indices stay 0-based on the device (`sampled`, `dead`): they only ever go back into the library.  Mirrored 1:1 by the
# tested Python (gaussiansplatting.jl_amd/mcmc.py).
struct GsrComposeGroup; src::Ptr{Cvoid}; dst::Ptr{Cvoid}; row_words::Int32; new_zero::Int32; end

# q (UInt32, N) and, unless `dead` is nothing, the dead mask (UInt8, N) of mcmc.jl:135-140
function mcmc_weights!(q, dead, opacities, scales; min_opacity::Float32 = 0f0, log_max_scale::Float32 = 0f0)
    n = size(opacities, 2)
    check(ccall((:gsr_mcmc_weights, LIB), Cint,
        (Int64, Int32, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{UInt32}, Ptr{UInt8}, Ptr{Cvoid}),
        n, size(scales, 1), dptr(opacities), dptr(scales), min_opacity, log_max_scale, dptr(UInt32, q), dptr(UInt8, dead), hipstream()))
    return q
end

# multinomial_sample (mcmc.jl:220-225) + the multiplicities of split_sampled! (:237-240): (sampled, counts, total) on the device
function mcmc_sample(q, m::Integer, seed::UInt32)
    n = length(q)
    sampled = AMDGPU.zeros(UInt32, m)
    counts = AMDGPU.zeros(Int32, n)
    total = AMDGPU.zeros(UInt64, 1)
    nb = ccall((:gsr_mcmc_sample_scratch_bytes, LIB), Csize_t, (Int64,), n)
    scratch = AMDGPU.zeros(UInt64, max(Int(nb) ÷ 8, 1))
    check(ccall((:gsr_mcmc_sample, LIB), Cint,
        (Int64, Ptr{UInt32}, Int64, UInt32, Ptr{UInt32}, Ptr{Int32}, Ptr{UInt64}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        n, dptr(UInt32, q), m, seed, dptr(UInt32, sampled), dptr(Int32, counts), dptr(UInt64, total),
        Ptr{Cvoid}(UInt(pointer(scratch))), nb, hipstream()))
    return sampled, counts, total
end

_binoms(strategy) = ROCArray(permutedims(strategy.binoms))   # the library reads binoms[n·n_max + k]: row-major

# split_sampled! (mcmc.jl:232-260) in place on every row with counts > 0
function mcmc_split_sampled!(strategy, gs, counts, binoms = _binoms(strategy))
    check(ccall((:gsr_mcmc_split_sampled, LIB), Cint,
        (Int64, Int32, Ptr{Int32}, Ptr{Float32}, Int32, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
        size(gs.points, 2), size(gs.scales, 1), dptr(Int32, counts), dptr(binoms), strategy.n_max, strategy.min_opacity,
        dptr(gs.opacities), dptr(gs.scales), hipstream()))
    return
end

# relocation_params (mcmc.jl:266-280) on device arrays of activated opacities and Int32 ratios
function mcmc_relocation_params(strategy, o, ratio, binoms = _binoms(strategy))
    new_o, coeff = similar(o), similar(o)
    check(ccall((:gsr_mcmc_relocation_params, LIB), Cint,
        (Int64, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Int32, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
        length(o), dptr(o), dptr(Int32, ratio), dptr(binoms), strategy.n_max, strategy.min_opacity, dptr(new_o), dptr(coeff), hipstream()))
    return new_o, coeff
end

_row_words(x) = Int32(length(x) ÷ size(x, ndims(x)))
_mcmc_arrays(gs) = (gs.points, gs.features_dc, gs.features_rest, gs.scales, gs.rotations, gs.opacities)
_mcmc_opts(o) = (o.points, o.features_dc, o.features_rest, o.scales, o.rotations, o.opacities)

# the row copies of relocate_gaussians! (mcmc.jl:153-172), in place: x[:, dead] = x[:, sampled]; the moments of both are zeroed
function mcmc_relocate_rows!(gs, optimizers, dead, sampled)
    groups = GsrComposeGroup[]
    vp(x) = Ptr{Cvoid}(UInt(pointer(x)))
    foreach(_mcmc_arrays(gs), _mcmc_opts(optimizers)) do x, opt
        isempty(x) && return
        rw = _row_words(x)
        push!(groups, GsrComposeGroup(C_NULL, vp(x), rw, 0), GsrComposeGroup(C_NULL, vp(opt.μ[1]), rw, 1),
              GsrComposeGroup(C_NULL, vp(opt.ν[1]), rw, 1))
    end
    gs.ids ≡ nothing || push!(groups, GsrComposeGroup(C_NULL, vp(gs.ids), 1, 0))
    check(ccall((:gsr_mcmc_relocate_rows, LIB), Cint,
        (Ptr{GsrComposeGroup}, Int32, Int64, Ptr{UInt32}, Ptr{UInt32}, Int64, Ptr{Cvoid}),
        groups, length(groups), size(gs.points, 2), dptr(UInt32, dead), dptr(UInt32, sampled), length(dead), hipstream()))
    return
end

# inject_noise! (mcmc.jl:288-325); `seed` must differ from step to step
function mcmc_inject_noise!(strategy, gs, points_lr::Float32, seed::UInt32; extent::Float32)
    n = size(gs.points, 2)
    n == 0 && return
    check(ccall((:gsr_mcmc_inject_noise, LIB), Cint,
        (Int64, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, UInt32, Ptr{Cvoid}),
        n, size(gs.scales, 1), dptr(gs.points), dptr(gs.opacities), dptr(gs.scales), dptr(gs.rotations),
        points_lr * strategy.noise_lr, 0.5f0 * strategy.max_scale * extent, seed, hipstream()))
    return
end

# regularization_loss (mcmc.jl:104-107) as a device scalar; with vopacities (1,N) / vscales (3,N) — what ∇rasterize wrote,
# w.r.t. the ACTIVATED values — its gradient is added onto them: steps with the regulariser on run ∇rasterize +
# mcmc_regularization!(...; vopacities, vscales) + trainer_tail_step! (the fused backward_trainer_tail! has no gradient arrays)
function mcmc_regularization!(strategy, opacities, scales; vopacities = nothing, vscales = nothing)
    n = size(opacities, 2)
    loss = AMDGPU.zeros(Float32, 1)
    nb = ccall((:gsr_mcmc_regularization_scratch_bytes, LIB), Csize_t, (Int64,), n)
    scratch = AMDGPU.zeros(UInt8, max(Int(nb), 4))
    check(ccall((:gsr_mcmc_regularization, LIB), Cint,
        (Int64, Int32, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        n, size(scales, 1), dptr(opacities), dptr(scales), strategy.opacity_reg, strategy.scale_reg, dptr(loss), dptr(vopacities),
        dptr(vscales), Ptr{Cvoid}(UInt(pointer(scratch))), Csize_t(length(scratch)), hipstream()))
    return loss
end

# Sketch of post_train_step! (mcmc.jl:109-124) on these entry points — the control flow of the reference, the tested form of
# which is mcmc.py's post_train_step.  `seeds` yields a fresh UInt32 per call (Python: (seed_base, counter) mixed as
# DefaultStrategy.next_split_seed does, separate counters for sampling and noise).  Appending the sampled rows is
# `append_gaussians!` of the reference on `gs.x[:, sampled .+ 1]`, or one gsr_compose_rows launch.
function mcmc_post_train_step!(strategy, gs, optimizers, seeds; step::Int, extent::Float32, points_lr::Float32)
    refining = strategy.start_refine < step < strategy.stop_refine && step % strategy.refine_every == 0
    if refining
        n = size(gs.points, 2)
        q, dead_mask = AMDGPU.zeros(UInt32, n), AMDGPU.zeros(UInt8, n)
        mcmc_weights!(q, dead_mask, gs.opacities, gs.scales; min_opacity = strategy.min_opacity,
                      log_max_scale = log(strategy.max_scale * extent))
        dead = UInt32.(findall(!iszero, dead_mask) .- 1)                      # read-back 1: the number of dead rows
        if 0 < length(dead) < n
            sampled, counts, total = mcmc_sample(q, length(dead), seeds())
            if Array(total)[1] > 0                                             # read-back 2
                mcmc_split_sampled!(strategy, gs, counts)
                mcmc_relocate_rows!(gs, optimizers, dead, sampled)
            end
        end
        n_new = min(strategy.max_cap, floor(Int, strategy.grow_factor * n)) - n
        if n_new > 0
            mcmc_weights!(q, nothing, gs.opacities, gs.scales)
            sampled, counts, total = mcmc_sample(q, n_new, seeds())
            if Array(total)[1] > 0
                mcmc_split_sampled!(strategy, gs, counts)
                ids = Int.(Array(sampled)) .+ 1
                GaussianSplatting.append_gaussians!(gs, optimizers;
                    new_points = gs.points[:, ids], new_features_dc = gs.features_dc[:, :, ids],
                    new_features_rest = isempty(gs.features_rest) ? gs.features_rest : gs.features_rest[:, :, ids],
                    new_scales = gs.scales[:, ids], new_rotations = gs.rotations[:, ids], new_opacities = gs.opacities[:, ids],
                    new_ids = gs.ids ≡ nothing ? nothing : gs.ids[ids])
            end
        end
    end
    mcmc_inject_noise!(strategy, gs, points_lr, seeds(); extent)
    return refining
end

# ---- the evaluation head (training.jl:487-532 `validate`; include/gsr.h: gsr_eval_*, gsr_frame_rgb8) ----

eval_scratch_bytes(w::Integer, h::Integer) = Int(ccall((:gsr_eval_scratch_bytes, LIB), Csize_t, (Int32, Int32), w, h))

"""
    eval_metrics!(out, image, target; sky_rgb = nothing, quantize = false, ssim_map = nothing, scratch = nothing)

`out` (4 Float32 on the device) <- (mean SSIM, MSE, PSNR, mean |x - y|) of the rgb channels of `image` (C, W, H) against
`target`: Float32 (W, H, 3) or UInt8 (3, W, H), as the dataset stores it.  `sky_rgb` (3, W, H) composites the dome behind the
frame first (`composite_sky`), `quantize` rounds to the 8-bit grid (`quantize8`), `ssim_map` (W, H, 3) receives the map.
What `validate` accumulates per view (training.jl:514-526), with nothing read back.
"""
function eval_metrics!(out, image, target; sky_rgb = nothing, quantize::Bool = false, ssim_map = nothing, scratch = nothing)
    c, w, h = size(image)
    scratch === nothing && (scratch = AMDGPU.zeros(UInt8, eval_scratch_bytes(w, h)))
    t32 = eltype(target) === UInt8 ? nothing : target
    t8 = eltype(target) === UInt8 ? target : nothing
    check(ccall((:gsr_eval_metrics, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}),
        w, h, c, dptr(image), dptr(sky_rgb), dptr(t32), dptr(UInt8, t8), quantize ? 1 : 0, dptr(ssim_map), dptr(out),
        dptr(Cvoid, scratch), hipstream()))
    return out
end

# `gl_texture` / `to_image` (rasterizer.jl:155-182) up to the bytes: rgb8 (3, W, H) UInt8 of the frame's colours
function frame_rgb8!(rgb8, image; sky_rgb = nothing, flip_rows::Bool = false)
    c, w, h = size(image)
    check(ccall((:gsr_frame_rgb8, LIB), Cint,
        (Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Int32, Ptr{UInt8}, Ptr{Cvoid}),
        w, h, c, dptr(image), dptr(sky_rgb), flip_rows ? 1 : 0, dptr(UInt8, rgb8), hipstream()))
    return rgb8
end

end # module
