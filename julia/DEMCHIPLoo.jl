# DEMCHIPLoo.jl -- included by DEMCHIP.jl (inside `module DEMCHIP`): the binding of include/demc_loo.h, the header that declares
# PSIS-LOO on the device.  Same status as DEMCHIP.jl: written against the header, checked against it statically
# (tests/test_loo_host.py), not executed here.

"the names of demc_loo's totals, in the order of total_out"
const LOO_TOTALS = (:elpd_loo, :se_elpd, :p_loo, :lppd, :looic, :n_k_high, :n_k_bad, :n_nonfinite)

"""
    loo(model::DEModel, de::DE, backend::HIPBackend, n_iter; model_spec::ModelSpec, pointwise=false)

The run of `sample`, followed by PSIS-LOO formed on the device (demc_loo, DESIGN.md 5.9): rows `offset+1 : offset+Ns` of
`bundle_samples` (src/main.jl:222-231, offset = burnin or 0), chains pooled.  Returns `(totals, table)`: `totals` a NamedTuple over
`LOO_TOTALS`; `table[i, :] = (elpd_loo_i, p_loo_i, khat_i, lppd_i, n_tail_i, l_cut_i)` of observation `i` in the order of the data
(`nothing` unless `pointwise`).  Served: the models `waic` serves; a window of more than 2^22 draws is refused with DEMC_EINVAL.
"""
function loo(model::DEModel, de::DE, b::HIPBackend, n_iter::Int; model_spec::ModelSpec, pointwise::Bool = false, kwargs...)
    groups = sample_init(model, de, n_iter)
    particles = vcat(groups...)
    P = length(particles); D = length(flatten(particles[1].Θ))
    cfg = make_config(de, D, n_iter, b)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = @ccall LIB.demc_create(Ref(cfg)::Ptr{DemcConfig}, href::Ptr{Ptr{Cvoid}})::Int32
    h = href[]
    N = isempty(model_spec.dims) ? 1 : Int(model_spec.dims[1])
    totals = Vector{Float64}(undef, 8)                                   # DEMC_LOO_NTOTAL
    table = pointwise ? Matrix{Float64}(undef, 6, N) : nothing           # C order [N][6]
    try
        check(h, rc)
        note(h)
        load_handle!(h, model_spec, de, particles)
        run_segments(de, n_iter, [h]) do first, count
            check(h, @ccall LIB.demc_step(h::Ptr{Cvoid}, Int64(first + de.n_initial)::Int64, Int32(count)::Int32)::Int32)
        end
        de.iter = n_iter + de.n_initial
        Ns = de.discard_burnin ? n_iter - de.burnin : n_iter
        offset = de.discard_burnin ? de.burnin : 0
        tp = pointwise ? pointer(table) : Ptr{Float64}(C_NULL)
        GC.@preserve table check(h, @ccall LIB.demc_loo(h::Ptr{Cvoid}, Int64(offset)::Int64, Int64(offset + Ns)::Int64, totals::Ptr{Float64},
            tp::Ptr{Float64})::Int32)
    finally
        h != C_NULL && @ccall LIB.demc_destroy(h::Ptr{Cvoid})::Int32
    end
    return NamedTuple{LOO_TOTALS}(Tuple(totals)), pointwise ? permutedims(table) : nothing
end

"""
    compare_loo(a, b) -> (elpd_diff, se_diff)

Two pointwise tables over the same data: `elpd_diff = sum(elpd_loo_a - elpd_loo_b)`, `se_diff = sqrt(N var(elpd_loo_a - elpd_loo_b))`.
"""
function compare_loo(a::Matrix{Float64}, b::Matrix{Float64})
    d = a[:, 1] .- b[:, 1]
    N = length(d)
    m = sum(d) / N
    return sum(d), sqrt(N * sum((d .- m) .^ 2) / (N - 1))
end
