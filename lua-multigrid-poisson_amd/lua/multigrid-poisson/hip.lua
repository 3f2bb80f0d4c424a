--[[
multigrid-poisson/hip.lua — drop-in GPU solver class for thenumbernine/lua-multigrid-poisson,
backed by libmgpoisson.so (include/mgpoisson.h) through LuaJIT FFI.

It accepts the constructor protocols of the reference:
  * cpu.lua table protocol (cpu.lua:173-216):
        local MG = require 'multigrid-poisson.hip'
        local mg = MG{size=n, maxiter=?, epsilon=?, errorCallback=function(iter, err) ... end, debug=?}
        mg:solve()            -- or mg:step() -> err
        mg:twoGrid(h, u, f)   -- u, f: lua-matrix-style 1-based tables u[i][j] (x = i), u updated in place
    mg.size is {n, n} (cpu.lua:178 matrix{size,size}); mg.smooth and mg.inPlaceIterativeSolver
    (MG.Jacobi | MG.GaussSeidel, cpu.lua:56-57) are writable: a change rebuilds the device context
    with psi and f kept.
  * cpu-raw.lua / gpu.lua positional protocol (cpu-raw.lua:142, 239; gpu.lua:26, 348):
        local mg = MG(size, real)    -- real = 'double' (default) or 'float'
        -- real = 'float' computes as cpu-raw.lua does (float images read into LuaJIT doubles: every
        -- expression in double, rounded at each store; arith = 'double'); MG{size=n, real='float',
        -- arith='real'} gives gpu.lua's float OpenCL arithmetic (gpu.lua:32), the table protocol's default
        mg:run()              -- two outer iterations, prints '#iter err'
        mg:twoGrid(h, uPtr, fPtr, L) -- raw real* host buffers of an L x L grid (cpu-raw.lua:186)
    Fields as cpu-raw.lua:148-171 names them, each an image-like {buffer=real*, width, height}
    downloaded on access: mg.psi, mg.f, mg.psiOld, mg.errorBuf, mg.tmpU, and per level size L
    mg.rs[L], mg.Rs[L], mg.vs[L], mg.Vs[L] (rs / vs computed on the device on request).
  * cpu-gpu.lua protocol (cpu-gpu.lua:55-72): MG(size, real, cpuDepth[, engine]) switches to the
    GPU's one-launch coarse engine at size 2^cpuDepth, or, given an engine with
    engine:twoGrid(h, uPtr, fPtr, L) (e.g. require'multigrid-poisson.cpu-raw'(2^cpuDepth)), hands
    that level's u and f to it and back, exactly as MultigridGPUSubset:twoGrid does.
  * Multi-GPU from this one Lua process (north_star: the V-cycle domain-decomposed across the
    node's GPUs): MG{size=n, dim=3, ngpu=8[, devices={...}], ...}.  The library builds the RCCL
    communicators (ncclCommInitAll) and runs every rank in its own host thread per call
    (mgp_group_*); fields are the global box.
mg:metrics() returns relErr, count, frobErr of the last outer iteration (gpu.lua:173-200);
mg:residualNorm() returns ||f - A psi||, ||f|| (device reduction).
real = 'mixed' (this build's addition; MG{size=n, real='mixed', ...} or MG(size, 'mixed')): mg.psi / mg.f are
double, and mg:step() is one step of mixed-precision defect correction (mgp_refine_step): the defect
f - A psi in double, mg.innerCycles (default 4) float cycles on it from a zero guess, psi = psi + e in
double; the err it returns is the double solver's (cpu.lua:203).  mg:solve() keeps cpu.lua:208-216's
loop over that step; mg:twoGrid raises; mg:refineResidual() returns ||f - A psi||, ||f|| of the double
fields.  One GPU only (ngpu > 1 raises).
Extra table fields select the build's configurations: dim (2|3), real, smoother ('jacobi'|'rbgs'|'gs_lex'),
cycle ('V'|'F'), prolong ('pc'|'linear'), coarse_init ('fresh'|'warm'), coarse_bc
('zero'|'consistent'|'face'|'neumann'), restriction ('average'|'full_weighting'), arith ('real'|'double'), device.
boundary = 'ghost' | 'face' | 'neumann' (this build's addition, default 'ghost' = the reference's box, the ghost cell
centre at 0): 'face' holds u = 0 on the box face, 'neumann' du/dn = 0 there (the ghost the reference carries commented
out, cpu.lua:28-31), on every level; an error together with a coarse_bc other than 'zero'.  Under 'neumann' psi is
determined up to a constant and f must sum to 0: mg:solve() removes f's mean before its first step and psi's after
its last one (mg:removeMean('f' | 'psi'), mgp_remove_mean); mg:step() does neither.
Defaults reproduce cpu.lua
(2D, double, Jacobi 7+7, V-cycle, injection, 2x2 average, fresh zero coarse guess, ghost value 0).
Errors from the library raise Lua errors (error()), as the reference's own failures do.

Not executable in this repository's CI (no Lua runtime in the image): tests/test_lua_binding.py
compiles the cdef below against include/mgpoisson.h, and ../mgpoisson/solver.py is the tested
Python twin of this file.
--]]
local ffi = require 'ffi'
local bit = require 'bit'

ffi.cdef[[
typedef struct mgp_ctx mgp_ctx;
typedef struct mgp_group mgp_group;
typedef struct mgp_opts {
    int32_t struct_size;
    int32_t dim;
    int64_t n[3];
    int32_t real_bytes;
    int32_t nu1, nu2;
    int32_t smoother;
    int32_t cycle;
    int32_t prolong;
    int32_t coarse_init;
    int32_t coarse_bc;
    int32_t coarse_sweeps;
    int32_t err_mode;
    int32_t device;
    int32_t rank, world;
    int32_t restriction;
    int64_t gather_cells;
    uint8_t comm_id[128];
    int32_t arith;
    int32_t api_version;
} mgp_opts;
int         mgp_version(void);
void        mgp_opts_default(mgp_opts* o);
int         mgp_create(mgp_ctx** out, const mgp_opts* o);
void        mgp_destroy(mgp_ctx* c);
const char* mgp_last_error(const mgp_ctx* c);
int         mgp_num_levels(const mgp_ctx* c);
int         mgp_level_info(const mgp_ctx* c, int level, int64_t info[8]);
int         mgp_init_point_charge(mgp_ctx* c);
int         mgp_set_field(mgp_ctx* c, int level, int which, const void* src, int64_t count, int mem);
int         mgp_get_field(const mgp_ctx* c, int level, int which, void* dst, int64_t count, int mem);
int         mgp_set_planes(mgp_ctx* c, int level, int which, int64_t z_begin, int64_t nz, const void* src, int mem);
int         mgp_get_planes(const mgp_ctx* c, int level, int which, int64_t z_begin, int64_t nz, void* dst, int mem);
int         mgp_cycle(mgp_ctx* c, double* err_out);
int         mgp_two_grid(mgp_ctx* c, double h, void* u, const void* f, int64_t L, int mem);
int         mgp_set_coarse_level(mgp_ctx* c, int64_t size);
typedef int (*mgp_coarse_fn)(void* user, double h, void* u, const void* f, int64_t size);
int         mgp_set_coarse_handoff(mgp_ctx* c, int64_t size, mgp_coarse_fn fn, void* user);
int         mgp_metrics(mgp_ctx* c, double* rel_err, int64_t* count, double* frob);
int         mgp_set_debug(mgp_ctx* c, int mode);
int         mgp_residual_norm(mgp_ctx* c, int level, double* rnorm, double* fnorm);
int         mgp_remove_mean(mgp_ctx* c, int level, int which, double* mean);
int         mgp_fmg_restrict_rhs(mgp_ctx* c, int level);
int         mgp_fmg_prolong(mgp_ctx* c, int level);
int         mgp_fmg(mgp_ctx* c, int32_t cycles_per_level, int32_t final_cycles, double* errs);
int         mgp_divergence(mgp_ctx* c, const void* vx, const void* vy, const void* vz, int mem);
int         mgp_gradient(mgp_ctx* c, int op, void* vx, void* vy, void* vz, int mem);
int         mgp_project(mgp_ctx* c, void* vx, void* vy, void* vz, int mem, int32_t fmg_cycles, int32_t cycles, double norms[2]);
int         mgp_set_coefficients(mgp_ctx* c, const void* bx, const void* by, const void* bz, int mem);
int         mgp_clear_coefficients(mgp_ctx* c);
int         mgp_has_coefficients(const mgp_ctx* c);
int         mgp_get_coefficients(const mgp_ctx* c, int level, int axis, void* dst, int64_t count, int mem);
int         mgp_refine_remove_mean(mgp_ctx* c, int which, double* mean);
int         mgp_group_remove_mean(mgp_group* g, int level, int which, double* mean);
int         mgp_batch_remove_mean(mgp_batch* b, int level, int which, double* means);
int         mgp_refine_begin(mgp_ctx* c);
int         mgp_refine_end(mgp_ctx* c);
int         mgp_refine_set(mgp_ctx* c, int which, const double* src, int64_t count, int mem);
int         mgp_refine_get(const mgp_ctx* c, int which, double* dst, int64_t count, int mem);
int         mgp_refine_residual(mgp_ctx* c, double* rnorm, double* fnorm);
int         mgp_refine_step(mgp_ctx* c, int32_t inner, double* rnorm, double* fnorm, double* err);
int         mgp_refine_solve(mgp_ctx* c, int32_t inner, double rtol, double epsilon, int32_t maxouter,
                             int32_t* steps, double* rel_hist, double* err_hist);
int         mgp_group_create(mgp_group** out, const mgp_opts* o, int ngpu, const int* devices);
mgp_ctx*    mgp_group_rank(mgp_group* g, int rank);
void        mgp_group_destroy(mgp_group* g);
const char* mgp_group_last_error(const mgp_group* g);
int         mgp_group_init_point_charge(mgp_group* g);
int         mgp_group_cycle(mgp_group* g, double* err_out);
int         mgp_group_cycles(mgp_group* g, int32_t k, double* errs);
int         mgp_group_set_field(mgp_group* g, int level, int which, const void* src, int64_t count, int mem);
int         mgp_group_get_field(mgp_group* g, int level, int which, void* dst, int64_t count, int mem);
int         mgp_group_residual_norm(mgp_group* g, int level, double* rnorm, double* fnorm);
typedef struct mgp_batch mgp_batch;
int         mgp_batch_create(mgp_batch** out, const mgp_opts* o, int32_t batch);
void        mgp_batch_destroy(mgp_batch* b);
const char* mgp_batch_last_error(const mgp_batch* b);
int         mgp_batch_size(const mgp_batch* b);
int         mgp_batch_plan(const mgp_opts* o, int32_t batch, int64_t* rows, int max_levels);
int         mgp_batch_init_point_charge(mgp_batch* b);
int         mgp_batch_set_field(mgp_batch* b, int member, int level, int which, const void* src, int64_t count, int mem);
int         mgp_batch_get_field(const mgp_batch* b, int member, int level, int which, void* dst, int64_t count, int mem);
int         mgp_batch_cycles(mgp_batch* b, int32_t k, double* errs);
int         mgp_batch_solve(mgp_batch* b, double epsilon, int32_t maxiter, int32_t* iters, double* last_err);
int         mgp_batch_residual_norm(mgp_batch* b, double* rnorm, double* fnorm);
int         mgp_batch_launches(const mgp_batch* b, int64_t* per_cycle);
int         mgp_batch_fmg_restrict_rhs(mgp_batch* b, int level);
int         mgp_batch_fmg_prolong(mgp_batch* b, int level);
int         mgp_batch_fmg(mgp_batch* b, int32_t cycles_per_level, int32_t final_cycles, double* errs);
int         mgp_batch_fmg_launches(const mgp_batch* b, int64_t* ascent);
int         mgp_batch_divergence(mgp_batch* b, int member, const void* vx, const void* vy, const void* vz, int mem);
int         mgp_batch_gradient(mgp_batch* b, int member, int op, void* vx, void* vy, void* vz, int mem);
int         mgp_batch_project(mgp_batch* b, void* vx, void* vy, void* vz, int mem, int32_t fmg_cycles, int32_t cycles, double* div_before, double* div_after);
]]

local lib = ffi.load(os.getenv('MGP_LIBRARY') or 'mgpoisson')

local CODES = {
	smoother = {jacobi = 0, rbgs = 1, gs_lex = 2},
	cycle = {V = 0, F = 1},
	prolong = {pc = 0, linear = 1},
	coarse_init = {fresh = 0, warm = 1},
	coarse_bc = {zero = 0, consistent = 1, face = 2, neumann = 3},
	restriction = {average = 0, full_weighting = 1},
	arith = {real = 0, double = 1},
}
-- include/mgpoisson.h MGP_FIELD_*; names of cpu-raw.lua:148-171
local FIELD = {psi = 0, f = 1, rs = 2, vs = 3, psiOld = 4, errorBuf = 5, tmpU = 6, Vs = 0, Rs = 1}

-- the `boundary` field of the table protocols -> boundary, coarse_bc
local function boundaryOf(a)
	local b = a.boundary or 'ghost'
	if b ~= 'ghost' and b ~= 'face' and b ~= 'neumann' then error("boundary: 'ghost' | 'face' | 'neumann'", 3) end
	if b == 'ghost' then return b, a.coarse_bc end
	if a.coarse_bc ~= nil and a.coarse_bc ~= 'zero' then
		error("boundary = '" .. b .. "' sets the boundary of every level: it does not combine with coarse_bc", 3)
	end
	return b, b
end

local function check(rc, ctx)
	if rc < 0 then error('libmgpoisson: ' .. ffi.string(lib.mgp_last_error(ctx)), 3) end
	return rc
end

local function checkGroup(rc, g)
	if rc < 0 then error('libmgpoisson: ' .. ffi.string(lib.mgp_group_last_error(g)), 3) end
	return rc
end

local MultigridHIP = {}
-- cpu.lua:56-57 inPlaceIterativeSolver values (functions there, markers here)
MultigridHIP.Jacobi = 'jacobi'
MultigridHIP.GaussSeidel = 'gs_lex'  -- cpu.lua:24-37's lexicographic in-place sweep, bit-identical (hyperplane order)
MultigridHIP.RedBlackGaussSeidel = 'rbgs'  -- the build's red/black form (the temporally blocked engines)

local LEVEL_FIELDS = {rs = true, Rs = true, vs = true, Vs = true}
local IMAGE_FIELDS = {psiOld = true, errorBuf = true, tmpU = true}

MultigridHIP.__index = function(self, k)
	if k == 'psi' or k == 'f' then
		if rawget(self, 'tableProtocol') then return self:getMatrix(FIELD[k]) end
		return self:getImage(FIELD[k], 0)
	end
	if k == 'psiBuffer' then return self:getBuffer(0) end
	if k == 'fBuffer' then return self:getBuffer(1) end
	if IMAGE_FIELDS[k] then return self:getImage(FIELD[k], 0) end
	if LEVEL_FIELDS[k] then
		local mg = self
		return setmetatable({}, {__index = function(_, L) return mg:getImage(FIELD[k], mg:levelOf(L)) end})
	end
	if k == 'inPlaceIterativeSolver' then
		return rawget(self, 'pendingSmoother') or rawget(self, 'build').smoother
	end
	-- the value last assigned, as a plain field of cpu.lua's object would read back
	if k == 'smooth' then return rawget(self, 'pendingSmooth') or rawget(self, 'build').smooth end
	return rawget(MultigridHIP, k)
end

MultigridHIP.__newindex = function(self, k, v)
	if k == 'smooth' then
		rawset(self, 'pendingSmooth', v)
	elseif k == 'inPlaceIterativeSolver' then
		local name = (v == MultigridHIP.GaussSeidel or v == 'GaussSeidel') and 'gs_lex' or
			((v == MultigridHIP.RedBlackGaussSeidel or v == 'RedBlackGaussSeidel') and 'rbgs' or
			((v == MultigridHIP.Jacobi or v == 'Jacobi') and 'jacobi' or
			error('inPlaceIterativeSolver: Jacobi | GaussSeidel | RedBlackGaussSeidel')))
		rawset(self, 'pendingSmoother', name)
	else
		rawset(self, k, v)
	end
end

-- class defaults (cpu.lua:18-22, cpu-raw.lua:121-124)
MultigridHIP.debug = false
-- cpu-raw.lua:121 / gpu.lua:21: check every phase's output for non-finite cells ("found a nan", cpu-raw.lua:135-139)
MultigridHIP.debugging = false
MultigridHIP.smooth = 7
MultigridHIP.epsilon = 1e-10
MultigridHIP.accuracy = 1e-10
MultigridHIP.maxiter = 1000
MultigridHIP.innerCycles = 4  -- this build's addition: float cycles per outer step of real = 'mixed'

setmetatable(MultigridHIP, {
	__call = function(cls, ...)
		local self = setmetatable({}, cls)
		self:init(...)
		return self
	end,
})

function MultigridHIP:makeOpts()
	local b = rawget(self, 'build')
	local n, dim = rawget(self, 'n'), rawget(self, 'dim')
	local o = ffi.new('mgp_opts')
	lib.mgp_opts_default(o)
	o.dim = dim
	o.n[0], o.n[1], o.n[2] = n, n, (dim == 3 and n or 1)
	o.real_bytes = (b.real == 'float' or b.real == 'mixed') and 4 or 8
	o.nu1, o.nu2 = b.smooth, b.smooth
	for field, map in pairs(CODES) do
		if b[field] ~= nil then o[field] = assert(map[b[field]], 'unknown ' .. field) end
	end
	if b.device then o.device = b.device end
	return o
end

function MultigridHIP:createContext()
	local o = self:makeOpts()
	local ngpu = rawget(self, 'ngpu')
	if ngpu and ngpu > 1 then
		local devs = rawget(self, 'devices')
		local darr = devs and ffi.new('int[?]', ngpu, devs) or nil
		local pp = ffi.new('mgp_group*[1]')
		checkGroup(lib.mgp_group_create(pp, o, ngpu, darr), nil)
		rawset(self, 'group', ffi.gc(pp[0], lib.mgp_group_destroy))
	else
		local pp = ffi.new('mgp_ctx*[1]')
		check(lib.mgp_create(pp, o), nil)
		rawset(self, 'ctx', ffi.gc(pp[0], lib.mgp_destroy))
		self:applyCoarse()
		-- real = 'mixed': double psi / f around the float cycles (mgp_destroy frees them with the context)
		if rawget(self, 'mixed') then check(lib.mgp_refine_begin(self.ctx), self.ctx) end
	end
end

-- cpu-gpu.lua:55-72 cpuDepth: the GPU's one-launch coarse engine from size 2^cpuDepth, or the hand-off of
-- that level to engine:twoGrid (re-applied whenever the context is rebuilt)
function MultigridHIP:applyCoarse()
	local cpuDepth, engine = rawget(self, 'cpuDepth'), rawget(self, 'engine')
	if not cpuDepth then return end
	local L = bit.lshift(1, cpuDepth)
	if engine then
		-- cpu-gpu.lua:17-52: the callback runs engine:twoGrid on the level's host copies
		local cb = rawget(self, 'handoff')
		if not cb then
			local pt = rawget(self, 'ptype')
			cb = ffi.cast('mgp_coarse_fn', function(user, h, u, f, size)
				local ok = pcall(engine.twoGrid, engine, h, ffi.cast(pt, u), ffi.cast(pt, f), tonumber(size))
				return ok and 0 or 1
			end)
			rawset(self, 'handoff', cb)  -- keep the callback alive
		end
		check(lib.mgp_set_coarse_handoff(self.ctx, L, cb, nil), self.ctx)
	else
		lib.mgp_set_coarse_level(self.ctx, L)  -- keeps the default switch when it does not fit
	end
end

function MultigridHIP:init(a, real, cpuDepth, engine)
	local args
	if type(a) == 'table' then
		args = a
		-- like cpu.lua:174-177: nil fields fall back to the class defaults
		rawset(self, 'tableProtocol', true)
		rawset(self, 'maxiter', args.maxiter)
		rawset(self, 'epsilon', args.epsilon)
		rawset(self, 'errorCallback', args.errorCallback)
		if args.debug ~= nil then rawset(self, 'debug', args.debug) end
	else
		-- cpu-raw.lua positional protocol: persistent coarse buffers (cpu-raw.lua:221) and, for
		-- real = 'float', its LuaJIT-double arithmetic over float images (cpu-raw.lua:142-153)
		-- (real = 'mixed' refines cycles of gpu.lua's float arithmetic: arith = 'real')
		args = {size = a, real = real, coarse_init = 'warm', arith = (real == 'mixed') and 'real' or 'double'}
		rawset(self, 'cpuDepth', cpuDepth)
		rawset(self, 'engine', engine)
	end
	local n = assert(tonumber(args.size), 'size is required')
	local dim = args.dim or 2
	rawset(self, 'real', args.real or 'double')
	rawset(self, 'mixed', args.real == 'mixed')
	if args.real == 'mixed' then
		if args.arith == 'double' then error("real = 'mixed': arith = 'double' is not offered", 2) end
		if args.ngpu and args.ngpu > 1 then error("real = 'mixed': one GPU only", 2) end
		if args.innerCycles then rawset(self, 'innerCycles', args.innerCycles) end
	end
	rawset(self, 'dim', dim)
	rawset(self, 'n', n)
	-- cpu.lua:178 self.size = matrix{size, size}; cpu-raw.lua:146 self.size = size
	rawset(self, 'size', rawget(self, 'tableProtocol') and {n, n} or n)
	rawset(self, 'ngpu', args.ngpu)
	rawset(self, 'devices', args.devices)
	local smoother = args.smoother
	if args.inPlaceIterativeSolver then
		local v = args.inPlaceIterativeSolver
		smoother = (v == MultigridHIP.GaussSeidel) and 'gs_lex' or
			((v == MultigridHIP.RedBlackGaussSeidel) and 'rbgs' or 'jacobi')
	end
	local boundary, bc = boundaryOf(args)
	rawset(self, 'boundary', boundary)
	rawset(self, 'build', {real = rawget(self, 'real'), smooth = args.smooth or MultigridHIP.smooth,
		smoother = smoother or 'jacobi', cycle = args.cycle, prolong = args.prolong,
		coarse_init = args.coarse_init, coarse_bc = bc, restriction = args.restriction,
		arith = args.arith, device = args.device})
	local cells = n * n * (dim == 3 and n or 1)
	rawset(self, 'count', cells)
	-- the context's real (real = 'mixed': a float context; its double psi / f are handled in get / setBuffer)
	local f32 = rawget(self, 'real') == 'float' or rawget(self, 'mixed')
	rawset(self, 'ctype', f32 and 'float[?]' or 'double[?]')
	rawset(self, 'ptype', f32 and 'float*' or 'double*')
	self:createContext()
	self:initPointCharge()
end

function MultigridHIP:initPointCharge()
	local g = rawget(self, 'group')
	if g then checkGroup(lib.mgp_group_init_point_charge(g), g)
	else check(lib.mgp_init_point_charge(self.ctx), self.ctx) end  -- cpu.lua:180-193
end

-- a changed smooth / inPlaceIterativeSolver takes effect here (the reference reads them inside
-- every twoGrid call, cpu.lua:96, 161): the context is rebuilt around the current psi and f
function MultigridHIP:applyKnobs()
	local ns, nm = rawget(self, 'pendingSmooth'), rawget(self, 'pendingSmoother')
	if ns == nil and nm == nil then return end
	local psi, f = self:getBuffer(0), self:getBuffer(1)
	local b = rawget(self, 'build')
	if ns ~= nil then b.smooth = ns end
	if nm ~= nil then b.smoother = nm end
	rawset(self, 'pendingSmooth', nil)
	rawset(self, 'pendingSmoother', nil)
	rawset(self, 'ctx', nil)
	rawset(self, 'group', nil)
	collectgarbage()
	self:createContext()
	self:setBuffer(0, psi)
	self:setBuffer(1, f)
end

-- the context that answers level queries: the solver's own, or rank 0's of a multi-GPU group
function MultigridHIP:infoCtx()
	local g = rawget(self, 'group')
	if g then return lib.mgp_group_rank(g, 0) end
	return self.ctx
end

function MultigridHIP:levelOf(size)
	local info = ffi.new('int64_t[8]')
	local ctx = self:infoCtx()
	local n = check(lib.mgp_num_levels(ctx), ctx)
	for l = 0, n - 1 do
		check(lib.mgp_level_info(ctx, l, info), ctx)
		if tonumber(info[0]) == size then return l end
	end
	error('no level of size ' .. tostring(size))
end

function MultigridHIP:metrics()
	if rawget(self, 'group') then error('metrics: single-GPU solvers only (ngpu > 1 runs mgp_group_*)', 2) end
	local rel, n, frob = ffi.new('double[1]'), ffi.new('int64_t[1]'), ffi.new('double[1]')
	check(lib.mgp_metrics(self.ctx, rel, n, frob), self.ctx)
	return rel[0], tonumber(n[0]), frob[0]
end

function MultigridHIP:residualNorm(level)
	local r, f = ffi.new('double[1]'), ffi.new('double[1]')
	local g = rawget(self, 'group')
	if g then checkGroup(lib.mgp_group_residual_norm(g, level or 0, r, f), g)
	else check(lib.mgp_residual_norm(self.ctx, level or 0, r, f), self.ctx) end
	return r[0], f[0]
end

-- subtract the mean of 'psi' or 'f' (level 0 by default) on the device; returns it (mgp_remove_mean)
function MultigridHIP:removeMean(which, level)
	local m = ffi.new('double[1]')
	local g = rawget(self, 'group')
	if rawget(self, 'mixed') and (level or 0) == 0 then
		check(lib.mgp_refine_remove_mean(self.ctx, FIELD[which or 'psi'], m), self.ctx)  -- MGP_REFINE_PSI / _F = 0 / 1
	elseif g then checkGroup(lib.mgp_group_remove_mean(g, level or 0, FIELD[which or 'psi'], m), g)
	else check(lib.mgp_remove_mean(self.ctx, level or 0, FIELD[which or 'psi'], m), self.ctx) end
	return m[0]
end

-- real = 'mixed': ||f - A psi||, ||f|| of the double fields
function MultigridHIP:refineResidual()
	local r, f = ffi.new('double[1]'), ffi.new('double[1]')
	check(lib.mgp_refine_residual(self.ctx, r, f), self.ctx)
	return r[0], f[0]
end

function MultigridHIP:getBuffer(which, level)
	level = level or 0
	local count = self.count
	if rawget(self, 'mixed') and level == 0 and which <= 1 then
		-- psi / f of real = 'mixed' are the double fields (MGP_REFINE_PSI = 0, MGP_REFINE_F = 1)
		local buf = ffi.new('double[?]', count)
		check(lib.mgp_refine_get(self.ctx, which, buf, count, 0), self.ctx)
		return buf, count
	end
	if level ~= 0 then
		-- a group's fields are the global box: nz_global (info[2]); one context's are its planes (info[3])
		local info = ffi.new('int64_t[8]')
		local ctx = self:infoCtx()
		check(lib.mgp_level_info(ctx, level, info), ctx)
		count = tonumber(info[0] * info[1] * (rawget(self, 'group') and info[2] or info[3]))
	end
	local buf = ffi.new(self.ctype, count)
	local g = rawget(self, 'group')
	if g then checkGroup(lib.mgp_group_get_field(g, level, which, buf, count, 0), g)
	else check(lib.mgp_get_field(self.ctx, level, which, buf, count, 0), self.ctx) end
	return buf, count
end

function MultigridHIP:setBuffer(which, buf)
	if rawget(self, 'mixed') then
		check(lib.mgp_refine_set(self.ctx, which, buf, self.count, 0), self.ctx)
		return
	end
	local g = rawget(self, 'group')
	if g then checkGroup(lib.mgp_group_set_field(g, 0, which, buf, self.count, 0), g)
	else check(lib.mgp_set_field(self.ctx, 0, which, buf, self.count, 0), self.ctx) end
end

-- image-like view (cpu-raw.lua's image(w,h,1,real) with .buffer), a host copy
function MultigridHIP:getImage(which, level)
	local buf, count = self:getBuffer(which, level)
	local w = math.floor(math.sqrt(count) + 0.5)
	if self.dim == 3 then w = math.floor(count ^ (1 / 3) + 0.5) end
	return {buffer = buf, width = w, height = w, count = count}
end

-- 1-based nested table m[i][j] with i = x (cpu.lua's matrix indexing), 2D only
function MultigridHIP:getMatrix(which)
	local buf = self:getBuffer(which)
	local n = self.n
	if self.dim ~= 2 then return buf end
	local m = {}
	for i = 1, n do
		local row = {}
		for j = 1, n do row[j] = tonumber(buf[(i - 1) + n * (j - 1)]) end
		m[i] = row
	end
	return m
end

-- cpu.lua:196-206
function MultigridHIP:step()
	self:applyKnobs()
	local err = ffi.new('double[1]')
	local g = rawget(self, 'group')
	if rawget(self, 'mixed') then
		check(lib.mgp_refine_step(self.ctx, self.innerCycles, nil, nil, err), self.ctx)
	elseif g then checkGroup(lib.mgp_group_cycle(g, err), g)
	else check(lib.mgp_cycle(self.ctx, err), self.ctx) end
	if self.debug then print('err', err[0]) end
	return err[0]
end

local function finite(x) return x == x and x ~= math.huge and x ~= -math.huge end

-- cpu.lua:208-216, break rules included
function MultigridHIP:solve()
	if self.debug then print('#iter', 'err') end
	local neumann = rawget(self, 'boundary') == 'neumann'
	if neumann then self:removeMean('f') end
	for iter = 1, self.maxiter do
		local err = self:step()
		if self.errorCallback and self.errorCallback(iter, err) then break end
		if err < self.epsilon or not finite(err) then break end
	end
	if neumann then self:removeMean('psi') end
end

-- full multigrid start (this build's addition, mgp_fmg): psi from f alone (f restricted down the hierarchy, the
-- coarsest level solved, per level the cubic prolongation and `cycles` cycles), then `final` outer iterations.
-- Returns the last one's err (nan for final = 0).  boundary = 'neumann': f's mean is removed first, psi's afterwards.
function MultigridHIP:fmg(cycles, final)
	if rawget(self, 'group') then error('fmg: single-GPU solvers only (ngpu > 1 runs mgp_group_*)', 2) end
	if rawget(self, 'mixed') then error("fmg: real = 'mixed' is not supported", 2) end
	self:applyKnobs()
	cycles, final = cycles or 1, final or 1
	local errs = ffi.new('double[?]', math.max(final, 1))
	local neumann = rawget(self, 'boundary') == 'neumann'
	if neumann then self:removeMean('f') end
	check(lib.mgp_fmg(self.ctx, cycles, final, errs), self.ctx)
	if neumann then self:removeMean('psi') end
	local err = final > 0 and errs[final - 1] or 0 / 0
	if self.debug then print('err', err) end
	return err
end

-- the pieces of the full multigrid start: f of level + 1 = R f of level; u of level = P3 u of level + 1
function MultigridHIP:fmgRestrictRhs(level) check(lib.mgp_fmg_restrict_rhs(self.ctx, level), self.ctx) end
function MultigridHIP:fmgProlong(level) check(lib.mgp_fmg_prolong(self.ctx, level), self.ctx) end

-- MAC-grid projection (this build's addition; include/mgpoisson.h has the definitions).  The face arrays are host
-- buffers of the solver's real type (ffi.new(mg.ctype, count)), lexicographic with x fastest: vx (n+1) n [n], vy
-- n (n+1) [n], vz n n (n+1) reals (3D only; nil in 2D); mg:faceCounts() returns the three counts.
local function projectionCtx(self, what)
	if rawget(self, 'group') then error(what .. ': single-GPU solvers only (ngpu > 1 runs mgp_group_*)', 3) end
	if rawget(self, 'mixed') then error(what .. ": real = 'mixed' is not supported", 3) end
	self:applyKnobs()
	return self.ctx
end

function MultigridHIP:faceCounts()
	local n = self.n
	local nz = self.dim == 3 and n or 1
	return (n + 1) * n * nz, n * (n + 1) * nz, self.dim == 3 and n * n * (nz + 1) or 0
end

-- f = D v (mgp_divergence)
function MultigridHIP:divergence(vx, vy, vz)
	local ctx = projectionCtx(self, 'divergence')
	check(lib.mgp_divergence(ctx, vx, vy, vz, 0), ctx)
end

-- subtract ~= false: v -= G psi in place; subtract = false: the buffers receive G psi (mgp_gradient)
function MultigridHIP:gradient(vx, vy, vz, subtract)
	local ctx = projectionCtx(self, 'gradient')
	check(lib.mgp_gradient(ctx, subtract == false and 0 or 1, vx, vy, vz, 0), ctx)
end

-- f = D v (its mean removed under boundary = 'neumann'), psi from a full multigrid start of `fmg` cycles per level and
-- `cycles` final ones (fmg = 0: `cycles` outer iterations from the stored psi), v -= G psi in place (mgp_project).
-- Returns ||D v||_2 before and after.
function MultigridHIP:project(vx, vy, vz, fmg, cycles)
	local ctx = projectionCtx(self, 'project')
	local norms = ffi.new('double[2]')
	check(lib.mgp_project(ctx, vx, vy, vz, 0, fmg or 1, cycles or 1, norms), ctx)
	return norms[0], norms[1]
end

-- Variable coefficients (this build's addition; include/mgpoisson.h has the definition): div(beta grad psi) = f with
-- positive face coefficients bx, by[, bz], host buffers laid out like the projection's faces (mg:faceCounts()).
function MultigridHIP:setCoefficients(bx, by, bz)
	local ctx = projectionCtx(self, 'setCoefficients')
	check(lib.mgp_set_coefficients(ctx, bx, by, bz, 0), ctx)
end

function MultigridHIP:clearCoefficients()
	local ctx = projectionCtx(self, 'clearCoefficients')
	check(lib.mgp_clear_coefficients(ctx), ctx)
end

function MultigridHIP:hasCoefficients()
	return lib.mgp_has_coefficients(projectionCtx(self, 'hasCoefficients')) == 1
end

-- level `level`'s faces of `axis` (0 x, 1 y, 2 z) into dst (count reals of the solver's real type)
function MultigridHIP:getCoefficients(level, axis, dst, count)
	local ctx = projectionCtx(self, 'getCoefficients')
	check(lib.mgp_get_coefficients(ctx, level, axis, dst, count, 0), ctx)
	return dst
end

-- cpu-raw.lua:239-258 / gpu.lua:348-373: two outer iterations
function MultigridHIP:run()
	if not rawget(self, 'group') then check(lib.mgp_set_debug(self.ctx, self.debugging and 1 or 0), self.ctx) end
	print('#iter', 'err')
	for iter = 1, 2 do
		local err = self:step()
		print(iter, err)
		if err < self.accuracy or not finite(err) then break end  -- gpu.lua:371 math.isfinite
	end
end

-- cpu-raw.lua:186 twoGrid(h, u, f, L) on raw host real* buffers (u updated in place), or
-- cpu.lua:70 twoGrid(h, u, f) on lua-matrix-style tables u[i][j] (x = i; u updated in place)
function MultigridHIP:twoGrid(h, u, f, L)
	self:applyKnobs()
	if rawget(self, 'mixed') then error("twoGrid: not offered with real = 'mixed' (level 0 is the refinement's scratch)", 2) end
	if type(u) == 'table' then
		local n = #u
		local ub, fb = ffi.new(self.ctype, n * n), ffi.new(self.ctype, n * n)
		for i = 1, n do
			for j = 1, n do
				ub[(i - 1) + n * (j - 1)] = u[i][j]
				fb[(i - 1) + n * (j - 1)] = f[i][j]
			end
		end
		check(lib.mgp_two_grid(self.ctx, h, ub, fb, n, 0), self.ctx)
		for i = 1, n do
			for j = 1, n do u[i][j] = tonumber(ub[(i - 1) + n * (j - 1)]) end
		end
		return u
	end
	check(lib.mgp_two_grid(self.ctx, h, u, f, L, 0), self.ctx)
end

-- MGBatch: `batch` independent boxes of one size in one hierarchy (mgp_batch_*; this build's addition, the reference
-- solves one box).  MultigridHIP.Batch{size = n, batch = B, dim = ?, real = ?, smooth = ?, ...} takes the build
-- fields of MultigridHIP's table protocol; every member starts as cpu.lua:180-193's point charge.  Buffers are raw
-- real* of B * n^dim elements (member slowest, then x fastest), or of n^dim for one member (0-based).  errorCallback
-- is not offered: the members stop on the device (cpu.lua:208-216 per member).  NOT EXECUTED here (no Lua runtime).
local MGBatch = {}
MGBatch.__index = MGBatch
MGBatch.smooth = MultigridHIP.smooth
MGBatch.epsilon = MultigridHIP.epsilon
MGBatch.maxiter = MultigridHIP.maxiter

local function checkBatch(rc, b)
	if rc < 0 then error('libmgpoisson: ' .. ffi.string(lib.mgp_batch_last_error(b)), 3) end
	return rc
end

setmetatable(MGBatch, {
	__call = function(cls, a)
		assert(a.errorCallback == nil, 'MGBatch: errorCallback is not offered (the members stop on the device)')
		local self = setmetatable({}, cls)
		self.n, self.dim, self.batch = assert(a.size), a.dim or 2, assert(a.batch)
		if a.maxiter ~= nil then self.maxiter = a.maxiter end
		if a.epsilon ~= nil then self.epsilon = a.epsilon end
		local boundary, bc = boundaryOf(a)
		self.boundary = boundary
		self.build = {real = a.real or 'double', smooth = a.smooth or cls.smooth,
			smoother = a.inPlaceIterativeSolver or a.smoother or 'jacobi', cycle = a.cycle, prolong = a.prolong,
			coarse_init = a.coarse_init, coarse_bc = bc, device = a.device}
		local o = MultigridHIP.makeOpts(self)
		local out = ffi.new('mgp_batch*[1]')
		checkBatch(lib.mgp_batch_create(out, o, self.batch), nil)
		self.handle = ffi.gc(out[0], lib.mgp_batch_destroy)
		self.ctype = o.real_bytes == 4 and 'float[?]' or 'double[?]'
		self.cells = self.n ^ self.dim
		self.iters = ffi.new('int32_t[?]', self.batch)
		self.err = ffi.new('double[?]', self.batch)
		self:initPointCharge()
		return self
	end,
})

function MGBatch:initPointCharge() checkBatch(lib.mgp_batch_init_point_charge(self.handle), self.handle) end

-- which: 'psi' | 'f' | 'psiOld' (get only); member nil = every member
function MGBatch:getBuffer(which, member, level)
	local count = (member and 1 or self.batch) * (level and level > 0 and (self.n / 2 ^ level) ^ self.dim or self.cells)
	local buf = ffi.new(self.ctype, count)
	checkBatch(lib.mgp_batch_get_field(self.handle, member or -1, level or 0, FIELD[which], buf, count, 0), self.handle)
	return buf, count
end

function MGBatch:setBuffer(which, buf, member, level, mem)
	local count = (member and 1 or self.batch) * (level and level > 0 and (self.n / 2 ^ level) ^ self.dim or self.cells)
	checkBatch(lib.mgp_batch_set_field(self.handle, member or -1, level or 0, FIELD[which], buf, count, mem or 0), self.handle)
end

-- cpu.lua:196-206 on every member, k times with one host synchronisation: errs[it * batch + m]
function MGBatch:cycles(k)
	local errs = ffi.new('double[?]', k * self.batch)
	checkBatch(lib.mgp_batch_cycles(self.handle, k, errs), self.handle)
	return errs
end

function MGBatch:step() return self:cycles(1) end

-- every member's own mean subtracted from its 'psi' or 'f' of a level; returns the B means
function MGBatch:removeMean(which, level)
	local m = ffi.new('double[?]', self.batch)
	checkBatch(lib.mgp_batch_remove_mean(self.handle, level or 0, FIELD[which or 'psi'], m), self.handle)
	return m
end

-- cpu.lua:208-216 per member: fills self.iters[m] and self.err[m] (boundary = 'neumann': f's mean removed first,
-- psi's after the solve)
function MGBatch:solve()
	if self.boundary == 'neumann' then self:removeMean('f') end
	checkBatch(lib.mgp_batch_solve(self.handle, self.epsilon, self.maxiter, self.iters, self.err), self.handle)
	if self.boundary == 'neumann' then self:removeMean('psi') end
end

function MGBatch:residualNorm()
	local r, f = ffi.new('double[?]', self.batch), ffi.new('double[?]', self.batch)
	checkBatch(lib.mgp_batch_residual_norm(self.handle, r, f), self.handle)
	return r, f
end

function MGBatch:launches()
	local n = ffi.new('int64_t[1]')
	checkBatch(lib.mgp_batch_launches(self.handle, n), self.handle)
	return tonumber(n[0])
end

-- full multigrid start of every member (mgp_batch_fmg; MultigridHIP:fmg per member): psi from f alone, then `final`
-- outer iterations; returns the errs of the last one (double[batch]; nil with final = 0).  boundary = 'neumann': every
-- member's f loses its mean first and its psi afterwards
function MGBatch:fmg(cycles, final)
	cycles, final = cycles or 1, final or 1
	if self.boundary == 'neumann' then self:removeMean('f') end
	local errs = ffi.new('double[?]', math.max(final, 1) * self.batch)
	checkBatch(lib.mgp_batch_fmg(self.handle, cycles, final, errs), self.handle)
	if self.boundary == 'neumann' then self:removeMean('psi') end
	if final < 1 then return nil end
	local last = ffi.new('double[?]', self.batch)
	for m = 0, self.batch - 1 do last[m] = errs[(final - 1) * self.batch + m] end
	return last
end

function MGBatch:fmgRestrictRhs(level) checkBatch(lib.mgp_batch_fmg_restrict_rhs(self.handle, level), self.handle) end
function MGBatch:fmgProlong(level) checkBatch(lib.mgp_batch_fmg_prolong(self.handle, level), self.handle) end

-- kernel launches of the last fmg() call's ascent (independent of batch)
function MGBatch:fmgLaunches()
	local n = ffi.new('int64_t[1]')
	checkBatch(lib.mgp_batch_fmg_launches(self.handle, n), self.handle)
	return tonumber(n[0])
end

-- MAC-grid projection of the members (mgp_batch_divergence / mgp_batch_gradient / mgp_batch_project): raw real* host
-- buffers, member slowest, then MultigridHIP:faceCounts() reals per member in MultigridHIP's layout (vz: 3D only, nil
-- in 2D); member nil = every member, otherwise that member (0-based) and one member's faces

-- every member's (or one member's) f = D v
function MGBatch:divergence(vx, vy, vz, member)
	checkBatch(lib.mgp_batch_divergence(self.handle, member or -1, vx, vy, vz, 0), self.handle)
end

-- subtract ~= false: v -= G psi in place; subtract = false: the buffers receive G psi
function MGBatch:gradient(vx, vy, vz, subtract, member)
	checkBatch(lib.mgp_batch_gradient(self.handle, member or -1, subtract == false and 0 or 1, vx, vy, vz, 0), self.handle)
end

-- MultigridHIP:project on every member in one call, in place: f = D v (each member's mean removed under boundary =
-- 'neumann'), psi from mgp_batch_fmg's path (fmg = 0: `cycles` outer iterations from the stored psi), v -= G psi.
-- Returns ||D v||_2 before and after per member (two double[batch])
function MGBatch:project(vx, vy, vz, fmg, cycles)
	local before, after = ffi.new('double[?]', self.batch), ffi.new('double[?]', self.batch)
	checkBatch(lib.mgp_batch_project(self.handle, vx, vy, vz, 0, fmg or 1, cycles or 1, before, after), self.handle)
	return before, after
end

MultigridHIP.Batch = MGBatch

return MultigridHIP
