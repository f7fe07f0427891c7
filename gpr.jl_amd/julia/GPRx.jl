"""
    GPRx — Julia ccall shim routing GaussianProcesses.jl's exact SE-ARD GP evaluations to the
    MI355X library (libgprx.so, C ABI in include/gprx.h).

Load it after GaussianProcesses (e.g. one `include` in src/GPR.jl, see INTEGRATION.md); the
experiment scripts (examples/noise.jl, examples/hyperparameter.jl) stay textually unchanged:

    GP(X, y, mean, SEArd(...))            -> gprx_gp_create + gprx_gp_lml   (CPnoise.jl:40)
    optimize!(gp, LBFGS(...), Options())  -> gprx_gp_lml / gprx_gp_lml_grad per evaluation
    predict_y(gp, x*)                     -> gprx_gp_predict                 (predictdynamics.jl:13)
    predict_f(gp, x*; full_cov=true)      -> gprx_gp_predict_cov
    rand(gp, x*, n)                       -> gprx_gp_sample (randn on the Julia side)
    predict_LOO(gp), logp_LOO(gp)         -> gprx_gp_loo
    dlogpdθ_LOO(gp)                       -> gprx_gp_loo_grad   [ext, recalled]
    predict_CVfold(gp, folds), logp_CVfold(gp, folds) -> gprx_gp_set_folds, gprx_gp_cvfold

plus `GPRx.optimize_all!(gps)`: the loop `for gp in gps; optimize!(gp, LBFGS(linesearch =
BackTracking(order=2)), Optim.Options(time_limit=10.)); end` of CPnoise.jl:37-43 as ONE
gprx_batch_optimize call (device LBFGS, every GP of the trial in lock-step).

Method names follow GaussianProcesses v0.12.4 internals (update_mll!, update_target_and_dtarget!,
predict_f); they are [ext] — confirm against that package's source before shipping.
Not executable in the build container (no Julia runtime).
"""
module GPRx

using GaussianProcesses
using GaussianProcesses: GPE, SEArd, Mean
using LinearAlgebra
using Random

const LIB = joinpath(@__DIR__, "..", "lib", "libgprx.so")
const ABI = Cint(3)  # include/gprx.h GPRX_ABI_VERSION these ccall signatures follow
const OK, NOT_PD, INVALID = Cint(0), Cint(1), Cint(2)

function __init__()
    abi = ccall((:gprx_abi_version, LIB), Cint, ())
    abi == ABI || error("gprx: $LIB implements ABI version $abi, GPRx.jl expects $ABI")
end

# one context (HIP stream) per Julia thread; device = thread mod #GPUs (core.jl:28 workers), the
# device count from the library (GPRX_NGPU, if set, caps it, e.g. to leave GPUs to other jobs)
const CTX = Dict{Int,Ptr{Cvoid}}()
function ndevices()
    n = Int(ccall((:gprx_device_count, LIB), Cint, ()))
    n > 0 || error("gprx: no visible GPU")
    haskey(ENV, "GPRX_NGPU") ? clamp(parse(Int, ENV["GPRX_NGPU"]), 1, n) : n
end
const CTX_LOCK = ReentrantLock()
function context()
    tid = Threads.threadid()
    lock(CTX_LOCK) do
        get!(CTX, tid) do
            ngpu = ndevices()
            h = Ref{Ptr{Cvoid}}(C_NULL)
            rc = ccall((:gprx_ctx_create, LIB), Cint, (Cint, Ref{Ptr{Cvoid}}), (tid - 1) % ngpu, h)
            rc == OK || error("gprx_ctx_create failed ($rc)")
            h[]
        end
    end
end

# device handle per GPE; X and y - μ(X) copied once (μ is θ-independent: MeanDynamics has no
# parameters, src/mDynamics.jl:29)
mutable struct Handle
    ptr::Ptr{Cvoid}
end
const HANDLES = WeakKeyDict{Any,Handle}()
const H_LOCK = ReentrantLock()

function handle(gp::GPE)
    lock(H_LOCK) do
        get!(HANDLES, gp) do
            X = Matrix{Float64}(gp.x)                      # d x N column-major, as the ABI
            r = gp.y .- GaussianProcesses.mean(gp.mean, X)
            h = Ref{Ptr{Cvoid}}(C_NULL)
            rc = ccall((:gprx_gp_create, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                       context(), X, size(X, 1), size(X, 2), r, h)
            rc == OK || error("gprx_gp_create failed ($rc)")
            hd = Handle(h[])
            finalizer(x -> ccall((:gprx_gp_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.ptr), hd)
            hd
        end
    end
end

# θ in GaussianProcesses' optimiser order: [logNoise; mean params (none); logℓ...; logσ]
theta(gp::GPE) = Float64[gp.logNoise.value; GaussianProcesses.get_params(gp.kernel)...]

# status -> the exception GaussianProcesses' own path raises; `info` is the 1-based failing pivot
# the ABI reports (LAPACK dpotrf's info, as cholesky! puts it into PosDefException)
function check(rc::Cint, gp, info::Integer=-1)
    rc == NOT_PD && throw(LinearAlgebra.PosDefException(Int(info)))
    rc == INVALID && throw(ArgumentError("gprx: invalid hyperparameters"))
    rc == OK || error("gprx device error ($rc)")
end

# One evaluation of the GP's batch of one (gprx_batch_run: it also reports the failing pivot).
# flags: 1 = gradient.  Afterwards gp.alpha holds K^-1 (y - m(X)) of the device factorisation.
function evaluate!(gp::GPE, flags::Integer)
    b = ccall((:gprx_gp_batch, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), handle(gp).ptr)
    m = Ref{Float64}(0.0)
    g = zeros(length(theta(gp)))
    st, info = Ref{Cint}(0), Ref{Cint}(0)
    rc = ccall((:gprx_batch_run, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Cuint, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ref{Cint}, Ref{Cint}),
               b, theta(gp), Cuint(flags), m, g, C_NULL, C_NULL, st, info)
    check(rc, gp, info[])
    a = zeros(length(gp.y))
    check(ccall((:gprx_batch_alpha, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), b, a), gp)
    gp.alpha = a
    return m[], g
end

# gp.cK (the host PDMat of K and its Cholesky factor) is not maintained by the device path: the
# factorisation stays in HBM.  Code that reads it directly calls
# materialize!(gp) first, which runs GaussianProcesses' own update_cK! / update_mll! on the host
# once at the current hyperparameters (O(N^3) on the CPU, on request only).
function materialize!(gp::GPE)
    invoke(GaussianProcesses.update_mll!, Tuple{GPE}, gp)
    gp
end

# The varargs absorb GaussianProcesses' optional positional arguments (e.g. the precompute buffer
# that optimize! passes to update_target_and_dtarget!) so these methods win dispatch for every
# call form.
function GaussianProcesses.update_mll!(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, args...; kwargs...)
    m, _ = evaluate!(gp, 0)
    gp.mll = m
    gp.target = gp.mll
    gp
end

function GaussianProcesses.update_target_and_dtarget!(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, args...; kwargs...)
    m, g = evaluate!(gp, 1)
    gp.mll = m
    gp.dmll = g
    gp.target = gp.mll
    gp.dtarget = g
    gp
end

function GaussianProcesses.predict_f(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, x::AbstractMatrix; full_cov::Bool=false)
    xs = Matrix{Float64}(x)
    M = size(xs, 2)
    if full_cov  # the M x M posterior covariance K** - V'V on the device (symmetric, not clamped)
        mu = zeros(M)
        cov = zeros(M, M)
        check(ccall((:gprx_gp_predict_cov, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}),
                    handle(gp).ptr, xs, M, mu, cov), gp)
        return mu .+ GaussianProcesses.mean(gp.mean, xs), cov
    end
    mu = zeros(M)
    var = zeros(M)
    check(ccall((:gprx_gp_predict, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{Float64}),
                handle(gp).ptr, xs, M, mu, var), gp)
    return mu .+ GaussianProcesses.mean(gp.mean, xs), var   # predict_y adds exp(2 logNoise)
end

# rand(gp, x, n): n draws of the posterior function at the columns of x, M x n.  The standard
# normals are drawn here (randn); the covariance, its factor (with gprx's own jitter ladder, see
# include/gprx.h) and mu + L z run on the device.  f-space plus the prior mean.
function Random.rand(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, x::AbstractMatrix, n::Int)
    xs = Matrix{Float64}(x)
    M = size(xs, 2)
    Z = randn(M, n)              # column s = one draw: the ABI's [S][M] row-major
    out = zeros(M, n)
    jit = Ref{Float64}(0.0)
    check(ccall((:gprx_gp_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ref{Float64}),
                handle(gp).ptr, xs, M, Z, n, out, jit), gp)
    return out .+ GaussianProcesses.mean(gp.mean, xs)
end
Random.rand(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, x::AbstractMatrix) = vec(rand(gp, x, 1))

# predict_LOO(gp), logp_LOO(gp) (GaussianProcesses crossvalidation.jl): the leave-one-out mean and
# variance at every training point and the summed log predictive density, from the device
# factorisation of the last evaluation (gprx_gp_loo: R&W 5.10-5.12 over diag(K^-1) and alpha).  The
# prior mean at the training inputs is added back here; the variance includes the noise.
function GaussianProcesses.predict_LOO(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd})
    N = length(gp.y)
    mu, var = zeros(N), zeros(N)
    check(ccall((:gprx_gp_loo, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                handle(gp).ptr, mu, var, C_NULL), gp)
    return mu .+ GaussianProcesses.mean(gp.mean, Matrix{Float64}(gp.x)), var
end
function GaussianProcesses.logp_LOO(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd})
    lp = Ref{Float64}(0.0)
    check(ccall((:gprx_gp_loo, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                handle(gp).ptr, C_NULL, C_NULL, lp), gp)
    return lp[]
end

# dlogpdθ_LOO(gp) [ext, recalled: GaussianProcesses crossvalidation.jl pairs logp_LOO with a gradient of
# this name; the package source was not available to confirm it]: the gradient of logp_LOO with respect
# to the hyper-parameters in get_params' order [logNoise, kernel...] (the prior mean has no parameters
# here), from the device factorisation of the last evaluation (gprx_gp_loo_grad: R&W 5.13 contracted
# against dK/dθ).  The batch form is gprx_batch_loo_grad.
function GaussianProcesses.dlogpdθ_LOO(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd})
    g = zeros(size(gp.x, 1) + 2)
    check(ccall((:gprx_gp_loo_grad, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                handle(gp).ptr, C_NULL, g), gp)
    return g
end
# predict_CVfold(gp, folds), logp_CVfold(gp, folds) (GaussianProcesses crossvalidation.jl): folds is a
# vector of 1-based index vectors that partition the training points.  Every fold's points are
# predicted jointly from the points outside it, from the device factorisation of the last evaluation
# (gprx_gp_set_folds / gprx_gp_cvfold: R&W 5.4.2 in block form over the folds' blocks of K^-1).
# Returns the mean (prior mean added back) and the y-space marginal variance of every point in the
# order of the training points, and the sum of the folds' log predictive probabilities.  Methods of
# GaussianProcesses' own functions, like predict_LOO above, so a script's predict_CVfold(gp, folds)
# reaches the device unchanged [ext, recalled: the names are crossvalidation.jl's; the package source
# was not available to confirm its return shapes].
function fold_ids(folds::AbstractVector{<:AbstractVector{<:Integer}}, N::Integer)
    ids = fill(Cint(-1), N)
    for (f, idx) in enumerate(folds), i in idx
        1 <= i <= N || throw(ArgumentError("fold $f: index $i out of range 1:$N"))
        ids[i] < 0 || throw(ArgumentError("fold $f overlaps an earlier fold at point $i"))
        ids[i] = Cint(f - 1)
    end
    all(>=(0), ids) || throw(ArgumentError("the folds do not cover every training point"))
    return ids
end
function set_folds!(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, folds)
    ids = fold_ids(folds, length(gp.y))
    check(ccall((:gprx_gp_set_folds, LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint), handle(gp).ptr, ids, length(folds)), gp)
end
function GaussianProcesses.predict_CVfold(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, folds)
    set_folds!(gp, folds)
    N = length(gp.y)
    mu, var = zeros(N), zeros(N)
    check(ccall((:gprx_gp_cvfold, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                handle(gp).ptr, mu, var, C_NULL, C_NULL), gp)
    return mu .+ GaussianProcesses.mean(gp.mean, Matrix{Float64}(gp.x)), var
end
function GaussianProcesses.logp_CVfold(gp::GPE{<:Any,<:Any,<:Mean,<:SEArd}, folds)
    set_folds!(gp, folds)
    lp = Ref{Float64}(0.0)
    check(ccall((:gprx_gp_cvfold, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                handle(gp).ptr, C_NULL, C_NULL, C_NULL, lp), gp)
    return lp[]
end
function loo_grad_batch(batch::Ptr{Cvoid}, B::Integer, d::Integer)
    logp, grad, status = zeros(B), zeros(d + 2, B), zeros(Cint, B)
    rc = ccall((:gprx_batch_loo_grad, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
               batch, logp, grad, status)
    return rc, logp, grad, status
end

# predictdynamicsmin (examples/utils/predictdynamics.jl:30-102) for all test observations of one
# trial in one device launch.  `gps` must be MeanZero GPEs evaluated on this thread's context (the
# experiment's own thread, core.jl:28).  Returns the (q_cur, q̇_last) per coordinate and
# trajectory; the caller builds the CState from q_cur as predictdynamics.jl:48-101 does.
const MECH = Dict("P1" => Cint(1), "P2" => Cint(2), "CP" => Cint(3), "FB" => Cint(4))
function rollout_min(etype::String, gps::Vector{<:GPE}, startobservations::Vector{Vector{Float64}},
                     steps::Integer; usesin::Bool=false, Δt::Real=0.01)
    haskey(MECH, etype) || throw(ArgumentError("Experiment $etype not supported!"))
    all(gp -> gp.mean isa MeanZero, gps) || error("gprx: device rollouts need MeanZero GPs")
    T = length(startobservations)
    nc = etype == "P1" ? 1 : 2
    fin = zeros(2nc, T)
    bs = [ccall((:gprx_gp_batch, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), handle(gp).ptr) for gp in gps]
    rc = ccall((:gprx_rollout_min, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                Ptr{Float64}, Ptr{Float64}),
               context(), MECH[etype], Cint(usesin), Float64(Δt), Cint(steps), Cint(1), bs, zeros(Cint, nc),
               Cint(T), zeros(Cint, T), reduce(hcat, startobservations), fin)
    check(rc, gps)
    return [fin[:, t] for t in 1:T]
end

# The same two rollouts with MeanDynamics GPs (predict_y = μ(obs) + k*ᵀα, src/mDynamics.jl:41-55) in
# one device launch each: the handles hold y - μ(X) (handle()), the device solves the physics mean
# at every step.  vi_regularizer: the impulses' regularisation of the physics step (1e-10 for the
# four-bar).  status 2 / a NaN column: a physics step failed (the reference throws); vi_status: OR
# of the per-step physics statuses.  Argument types follow include/gprx.h; like the rest of this
# file they have not been run (no Julia runtime in the build container).
vi_regularizer(etype::String) = etype == "FB" ? 1e-10 : 0.0

# predictdynamicsmin (examples/utils/predictdynamics.jl:30-102) with MeanDynamics GPs
function rollout_min_md(etype::String, gps::Vector{<:GPE}, startobservations::Vector{Vector{Float64}},
                        steps::Integer; usesin::Bool=false, Δt::Real=0.01)
    haskey(MECH, etype) || throw(ArgumentError("Experiment $etype not supported!"))
    any(gp -> gp.mean isa MeanZero, gps) && error("gprx: MeanZero GPs roll out through rollout_min")
    T = length(startobservations)
    nc = etype == "P1" ? 1 : 2
    fin = zeros(2nc, T)
    status, vi_status = zeros(Cint, T), zeros(Cint, T)
    bs = [ccall((:gprx_gp_batch, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), handle(gp).ptr) for gp in gps]
    rc = ccall((:gprx_rollout_min_md, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Cdouble, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}),
               context(), MECH[etype], Cint(usesin), Float64(Δt), Cint(steps), vi_regularizer(etype), Cint(1), bs,
               zeros(Cint, nc), Cint(T), zeros(Cint, T), reduce(hcat, startobservations), fin, status, vi_status)
    check(rc, gps)
    return [fin[:, t] for t in 1:T], status, vi_status
end

# predictdynamics (examples/utils/predictdynamics.jl:7-22) with MeanDynamics GPs for all test CStates
# of one trial: gps[g] predicts CState position vωindices[g] (1-based, as the experiments' getvω)
function rollout_max_md(etype::String, gps::Vector{<:GPE}, startobservations::Vector{Vector{Float64}},
                        steps::Integer, vωindices::Vector{<:Integer}; regularizer::Real=0.0, Δt::Real=0.01)
    haskey(MECH, etype) || throw(ArgumentError("Experiment $etype not supported!"))
    any(gp -> gp.mean isa MeanZero, gps) && error("gprx: MeanZero GPs roll out through gprx_rollout_max")
    length(gps) == length(vωindices) || throw(ArgumentError("one GP per vω index"))
    T, G = length(startobservations), length(gps)
    d = length(startobservations[1])
    fin, perr = zeros(d, T), zeros(T)
    status, vi_status = zeros(Cint, T), zeros(Cint, T)
    bs = [ccall((:gprx_gp_batch, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), handle(gp).ptr) for gp in gps]
    rc = ccall((:gprx_rollout_max_md, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cdouble, Cint, Cdouble, Cdouble, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}),
               context(), MECH[etype], Float64(Δt), Cint(steps), Float64(regularizer), vi_regularizer(etype), Cint(1), bs,
               zeros(Cint, G), Cint(G), Vector{Cint}(vωindices), Cint(T), zeros(Cint, T),
               reduce(hcat, startobservations), fin, perr, status, vi_status)
    check(rc, gps)
    return [fin[:, t] for t in 1:T], perr, status, vi_status
end

# ---- the recorded rollouts (gprx_rollout_*_rec): the trajectory at the storage indices `record`
# (1-based: 1 the start, j the state after j - 1 steps; a vector for every trajectory or one per
# trajectory; nothing = every index 1:steps+1), in launches of at most `steps_per_launch` steps (0: the
# library's default).  The final outputs are those of the one-launch calls.  Like the rest of this
# file they have not been run.
function record_matrix(record, T::Integer, steps::Integer)
    rec = record === nothing ? collect(1:steps+1) : record
    R = rec isa AbstractVector{<:Integer} ? reduce(hcat, [Vector{Cint}(rec) for _ in 1:T]) : reduce(hcat, [Vector{Cint}(r) for r in rec])
    size(R, 2) == T || throw(ArgumentError("one record list per trajectory"))
    all(1 .<= R .<= steps + 1) && all(diff(R, dims=1) .>= 0) || throw(ArgumentError("record: non-decreasing indices in 1:steps+1"))
    return Matrix{Cint}(R)   # R x T column-major: trajectory t's indices contiguous, the ABI's rec[t*R ...]
end
trajectories(traj::Array{Float64,3}) = [[traj[:, r, t] for r in 1:size(traj, 2)] for t in 1:size(traj, 3)]

# predictdynamicsmin keeping (q_old, q̇_old) per coordinate at every recorded index; MeanZero or
# MeanDynamics GPs.  Returns (trajectories, final, status, vi_status), the last two nothing for MeanZero.
function rollout_min(etype::String, gps::Vector{<:GPE}, startobservations::Vector{Vector{Float64}}, steps::Integer,
                     record; usesin::Bool=false, Δt::Real=0.01, steps_per_launch::Integer=0)
    haskey(MECH, etype) || throw(ArgumentError("Experiment $etype not supported!"))
    md = !any(gp -> gp.mean isa MeanZero, gps)
    md || all(gp -> gp.mean isa MeanZero, gps) || error("gprx: a rollout's GPs share one mean type")
    T = length(startobservations)
    nc = etype == "P1" ? 1 : 2
    rec = record_matrix(record, T, steps)
    R = size(rec, 1)
    fin, traj = zeros(2nc, T), zeros(2nc, R, T)
    status, vi_status = zeros(Cint, T), zeros(Cint, T)
    bs = [ccall((:gprx_gp_batch, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), handle(gp).ptr) for gp in gps]
    if md
        rc = ccall((:gprx_rollout_min_md_rec, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Cdouble, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Ptr{Float64}),
                   context(), MECH[etype], Cint(usesin), Float64(Δt), Cint(steps), vi_regularizer(etype), Cint(1), bs,
                   zeros(Cint, nc), Cint(T), zeros(Cint, T), reduce(hcat, startobservations), fin, status, vi_status,
                   Cint(R), rec, Cint(steps_per_launch), traj)
    else
        rc = ccall((:gprx_rollout_min_rec, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Cdouble, Cint, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                    Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cint}, Cint, Ptr{Float64}),
                   context(), MECH[etype], Cint(usesin), Float64(Δt), Cint(steps), Cint(1), bs, zeros(Cint, nc),
                   Cint(T), zeros(Cint, T), reduce(hcat, startobservations), fin, Cint(R), rec, Cint(steps_per_launch), traj)
    end
    check(rc, gps)
    return trajectories(traj), [fin[:, t] for t in 1:T], md ? status : nothing, md ? vi_status : nothing
end

# predictdynamics (examples/utils/predictdynamics.jl:7-22) for all start CStates of one trial on the
# device, MeanZero or MeanDynamics GPs; gps[g] predicts CState position vωindices[g].  With the
# `record` keyword (see above; examples/energy.jl keeps every step: record = 2:steps+1) the CStates
# `oldstates` of predictdynamics.jl:18 at the recorded indices come first in the returned tuple:
# ([trajectories,] final CStates, projection errors, status, vi_status (nothing for MeanZero)).
function predictdynamics(etype::String, gps::Vector{<:GPE}, startobservations::Vector{Vector{Float64}},
                         steps::Integer, vωindices::Vector{<:Integer}; regularizer::Real=0.0, Δt::Real=0.01,
                         record=missing, steps_per_launch::Integer=0)
    haskey(MECH, etype) || throw(ArgumentError("Experiment $etype not supported!"))
    md = !any(gp -> gp.mean isa MeanZero, gps)
    md || all(gp -> gp.mean isa MeanZero, gps) || error("gprx: a rollout's GPs share one mean type")
    length(gps) == length(vωindices) || throw(ArgumentError("one GP per vω index"))
    T, G = length(startobservations), length(gps)
    d = length(startobservations[1])
    keep = record !== missing
    rec = keep ? record_matrix(record, T, steps) : zeros(Cint, 0, T)
    R = size(rec, 1)
    fin, perr, traj = zeros(d, T), zeros(T), zeros(d, R, T)
    status, vi_status = zeros(Cint, T), zeros(Cint, T)
    bs = [ccall((:gprx_gp_batch, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), handle(gp).ptr) for gp in gps]
    recp, trajp = R > 0 ? (pointer(rec), pointer(traj)) : (Ptr{Cint}(C_NULL), Ptr{Float64}(C_NULL))
    GC.@preserve rec traj begin
        if md
            rc = ccall((:gprx_rollout_max_md_rec, LIB), Cint,
                       (Ptr{Cvoid}, Cint, Cdouble, Cint, Cdouble, Cdouble, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                        Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint},
                        Cint, Ptr{Cint}, Cint, Ptr{Float64}),
                       context(), MECH[etype], Float64(Δt), Cint(steps), Float64(regularizer), vi_regularizer(etype), Cint(1), bs,
                       zeros(Cint, G), Cint(G), Vector{Cint}(vωindices), Cint(T), zeros(Cint, T),
                       reduce(hcat, startobservations), fin, perr, status, vi_status, Cint(R), recp, Cint(steps_per_launch), trajp)
        else
            rc = ccall((:gprx_rollout_max_rec, LIB), Cint,
                       (Ptr{Cvoid}, Cint, Cdouble, Cint, Cdouble, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Cint, Ptr{Cint},
                        Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Ptr{Float64}),
                       context(), MECH[etype], Float64(Δt), Cint(steps), Float64(regularizer), Cint(1), bs,
                       zeros(Cint, G), Cint(G), Vector{Cint}(vωindices), Cint(T), zeros(Cint, T),
                       reduce(hcat, startobservations), fin, perr, status, Cint(R), recp, Cint(steps_per_launch), trajp)
        end
    end
    check(rc, gps)
    out = ([fin[:, t] for t in 1:T], perr, status, md ? vi_status : nothing)
    return keep ? (trajectories(traj), out...) : out
end

# gprx_opt_options (include/gprx.h): same field order and C layout
struct OptOptions
    m::Cint
    iterations::Cint
    max_evals::Cint
    ls_iterations::Cint
    scaleinvH0::Cint
    refit::Cint
    successive_f_tol::Cint
    g_abstol::Cdouble
    time_limit::Cdouble
    alphaguess::Cdouble
    c_1::Cdouble
    rho_hi::Cdouble
    rho_lo::Cdouble
end
const OBJ_MLL, OBJ_LOO = Cint(0), Cint(1)  # include/gprx.h GPRX_OBJ_MLL, GPRX_OBJ_LOO
const STOP = ("iterations", "g_tol", "x_tol", "f_tol", "linesearch", "max_evals", "time_limit", "nan_gradient")

# optimize! for every GP of a trial (CPnoise.jl:37-43) in one device call: Optim LBFGS +
# BackTracking(order=2) as k_lbfgs, one lock-step evaluation of all GPs per round.  `time_limit`
# is per call (the reference's 10 s applies to each GP in turn).  Afterwards every GP holds its
# minimiser (set_params! + update_mll!, as optimize! leaves it).  Returns one NamedTuple per GP.
# objective = :mll minimises -mll (gprx_batch_optimize); :loo minimises -logp_LOO with dlogpdθ_LOO's
# gradient on the same device state machine (gprx_batch_optimize_obj with GPRX_OBJ_LOO), and
# `minimum` is then -logp_LOO at the minimiser.
function optimize_all!(gps::Vector{<:GPE}; time_limit::Real=NaN, iterations::Integer=1000,
                       max_evals::Integer=-1, g_abstol::Real=1e-8, objective::Symbol=:mll)
    objective in (:mll, :loo) || throw(ArgumentError("objective must be :mll or :loo, not $(repr(objective))"))
    obj = objective == :loo ? OBJ_LOO : OBJ_MLL
    B = length(gps)
    X1 = Matrix{Float64}(gps[1].x)
    d, N = size(X1)
    shared = all(gp -> gp.x == gps[1].x, gps)
    X = shared ? X1 : reduce(hcat, [Matrix{Float64}(gp.x) for gp in gps])
    Y = reduce(hcat, [gp.y .- GaussianProcesses.mean(gp.mean, Matrix{Float64}(gp.x)) for gp in gps])
    th0 = reduce(hcat, [theta(gp) for gp in gps])          # (d+2) x B: slot b's theta contiguous
    ctx = context()
    b = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gprx_batch_create, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
               ctx, B, d, N, 0, b)
    rc == OK || error("gprx_batch_create failed ($rc)")
    try
        rc = ccall((:gprx_batch_set_train, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Cint),
                   b[], X, shared ? 0 : d * N, Y, N, 0)
        rc == OK || error("gprx_batch_set_train failed ($rc)")
        o = Ref{OptOptions}()
        ccall((:gprx_opt_defaults, LIB), Cvoid, (Ref{OptOptions},), o)
        o[] = OptOptions(o[].m, iterations, max_evals, o[].ls_iterations, o[].scaleinvH0, 0, o[].successive_f_tol,
                         g_abstol, time_limit, o[].alphaguess, o[].c_1, o[].rho_hi, o[].rho_lo)
        thx = similar(th0)
        fmin = zeros(B)
        its, fc, gc, stp = (zeros(Cint, B) for _ in 1:4)
        rounds = Ref{Cint}(0)
        if obj == OBJ_MLL
            rc = ccall((:gprx_batch_optimize, LIB), Cint,
                       (Ptr{Cvoid}, Ptr{Float64}, Ref{OptOptions}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint},
                        Ptr{Cint}, Ptr{Cint}, Ref{Cint}),
                       b[], th0, o, thx, fmin, its, fc, gc, stp, rounds)
        else
            rc = ccall((:gprx_batch_optimize_obj, LIB), Cint,
                       (Ptr{Cvoid}, Cint, Ptr{Float64}, Ref{OptOptions}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint},
                        Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ref{Cint}),
                       b[], obj, th0, o, thx, fmin, its, fc, gc, stp, rounds)
        end
        rc == OK || error("gprx_batch_optimize failed ($rc)")
        for (k, gp) in enumerate(gps)   # optimize!: set_params!(gp, minimizer); update_target!(gp)
            GaussianProcesses.set_params!(gp, thx[:, k])
            GaussianProcesses.update_mll!(gp)
        end
        return [(minimizer=thx[:, k], minimum=fmin[k], iterations=Int(its[k]), f_calls=Int(fc[k]),
                 g_calls=Int(gc[k]), converged=(stp[k] & 0x100) != 0, stopped_by=STOP[(stp[k] & 0xff) + 1])
                for k in 1:B]
    finally
        ccall((:gprx_batch_destroy, LIB), Cvoid, (Ptr{Cvoid},), b[])
    end
end

end # module
