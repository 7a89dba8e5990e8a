'use strict';
// snarkjs-compatible PLONK API on the MI355X prover (SURVEY.md §8b).
//
// Drop-in for the two calls the reference's callers make into snarkjs 0.4.12
// (/root/reference/package.json:18; the dapp and the `snarkjs plonk prove|fullprove`
// CLI, README.md:50-53):
//   plonk.prove(zkeyFileName, witnessFileName, logger)       -> Promise<{proof, publicSignals}>
//   plonk.fullProve(input, wasmFile, zkeyFileName, logger)   -> Promise<{proof, publicSignals}>
// File arguments accept a path, a Buffer/Uint8Array, or {type: "mem", data}.
// Blinding scalars are drawn like snarkjs's Fr.random() unless options.blinding
// (11 x 32-byte LE Buffer) is given -- fixed blinding makes proofs bit-reproducible.
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');

// proof streams need more than HIP's default 4 hardware queues per process (kernels of
// independent streams sharing a queue serialise); read when HIP initialises
if ((process.env.GPU_MAX_HW_QUEUES || '4') === '4') process.env.GPU_MAX_HW_QUEUES = '24';
const addon = require(path.join(__dirname, 'build', 'nzcb.node'));

const R = BigInt('21888242871839275222246405745257275088548364400416034343698204186575808495617');
const BLINDING_BYTES = 11 * 32;

// File arguments: a path, {type: "mem", data}, or a Buffer / Uint8Array (used in place,
// not copied)
function readBin(x) {
  if (typeof x === 'string') return fs.readFileSync(x);
  if (x && x.type === 'mem') return Array.isArray(x.data) ? Buffer.from(x.data) : readBin(x.data);
  if (Buffer.isBuffer(x)) return x;
  if (x instanceof Uint8Array) return Buffer.from(x.buffer, x.byteOffset, x.byteLength);
  throw new Error('expected a file name, a buffer or {type: "mem", data}');
}

function randomBlinding() {
  const out = Buffer.alloc(BLINDING_BYTES);
  const mask = (BigInt(1) << BigInt(254)) - BigInt(1);
  for (let i = 0; i < 11; i++) {
    let v;
    do {
      v = BigInt('0x' + crypto.randomBytes(32).toString('hex')) & mask;
    } while (v >= R);
    for (let j = 0; j < 32; j++) {
      out[32 * i + j] = Number(v & BigInt(255));
      v >>= BigInt(8);
    }
  }
  return out;
}

// One HBM-resident context per (zkey, device): the zkey is uploaded once. A file name is
// memory-mapped by the library (nzcb_ctx_create_file), so zkeys of nzcp_live size
// (~3.9 GB, beyond a Node Buffer) work; buffers are keyed by content. A context has
// `lanes` proof lanes: concurrent prove / fullProve promises on it run on different lanes at
// the same time. options.lanes (or NZCB_LANES) asks for an exact count; by default the
// context takes up to 5 (bench.py's measured best) as far as the device's free HBM allows
// (~6.5 GB per extra lane at n = 2^21): a lane count that does not fit is rolled back by
// the library and the next smaller one is tried.
const DEFAULT_LANES = 5;
const ENV_LANES = process.env.NZCB_LANES ? Number(process.env.NZCB_LANES) : 0;
const contexts = new Map();
// Buffer -> {hash, probe}: the content hash is computed once per Buffer; a cheap probe
// (length, head and tail bytes) is checked on every lookup, so a caller that reuses one
// Buffer for another zkey or program gets it hashed again rather than the old context.
// Mutating a Buffer in the middle is not detected: pass a fresh Buffer for new contents.
const bufHashes = new WeakMap();
function probeOf(buf) {
  const k = Math.min(buf.length, 4096);
  return crypto.createHash('sha1').update(buf.subarray(0, k)).update(buf.subarray(buf.length - k))
    .update(String(buf.length)).digest('hex');
}
function contentHash(buf) {
  const probe = probeOf(buf);
  const e = bufHashes.get(buf);
  if (e && e.probe === probe) return e.hash;
  const hash = crypto.createHash('sha256').update(buf).digest('hex');
  bufHashes.set(buf, { hash, probe });
  return hash;
}
function setLanesFitting(ctx, want) {
  for (let l = want; ; l--) {
    try {
      return addon.setLanes(ctx, l);
    } catch (e) {
      if (l <= 1) throw e;
    }
  }
}
function contextFor(zkey, device, lanes) {
  let key;
  if (typeof zkey === 'string') {
    const st = fs.statSync(zkey);
    key = `file:${path.resolve(zkey)}:${st.size}:${st.mtimeMs}:${device}`;
  } else {
    key = contentHash(readBin(zkey)) + ':' + device;
  }
  lanes = lanes || ENV_LANES;
  let c = contexts.get(key);
  if (!c) {
    const ctx = typeof zkey === 'string' ? addon.createContextFile(zkey, device) : addon.createContext(readBin(zkey), device);
    try {
      c = { ctx, lanes: lanes ? addon.setLanes(ctx, lanes) : setLanesFitting(ctx, DEFAULT_LANES) };
    } catch (e) {
      addon.releaseContext(ctx);  // its HBM now, not at garbage collection
      throw e;
    }
    contexts.set(key, c);
  } else if (lanes && lanes !== c.lanes) {
    // a change of lane count waits for the proofs in flight (it rebuilds the lane pool)
    addon.setLanes(c.ctx, lanes);
    c.lanes = lanes;
  }
  return c.ctx;
}

function loggerFn(logger) {
  if (!logger) return null;
  if (typeof logger === 'function') return logger;
  if (typeof logger.debug === 'function') return (m) => logger.debug(m);
  return null;
}

async function prove(zkeyFileName, witnessFileName, logger, options) {
  options = options || {};
  const wtns = readBin(witnessFileName);
  const ctx = contextFor(zkeyFileName, options.device || 0, options.lanes);
  const res = await addon.prove(ctx, wtns, blindingFor(options), loggerFn(logger));
  return { proof: JSON.parse(res.proof), publicSignals: JSON.parse(res.publicSignals) };
}

function blindingFor(options) {
  const blinding = options.blinding ? Buffer.from(options.blinding) : randomBlinding();
  if (blinding.length !== BLINDING_BYTES) throw new Error('blinding must be 11 x 32 bytes');
  return blinding;
}

// ---------------------------------------------------------------------------
// Witness calculation from a circom 2.0.x witness .wasm (circom_runtime 0.1.17
// WitnessCalculatorBuilder / calculateWTNSBin interface, SURVEY.md §2 [EXT]).
// Parity unpinned: no circom artefact exists offline to test against.
// ---------------------------------------------------------------------------
function fnvHash(str) {
  const M = BigInt(2) ** BigInt(64);
  let h = BigInt('0xCBF29CE484222325');
  for (let i = 0; i < str.length; i++) {
    h ^= BigInt(str.charCodeAt(i));
    h = (h * BigInt('0x100000001B3')) % M;
  }
  return h.toString(16).padStart(16, '0');
}

function flatArray(a) {
  const res = [];
  (function fill(x) {
    if (Array.isArray(x)) x.forEach(fill);
    else res.push(x);
  })(a);
  return res;
}

async function wtnsCalculate(input, wasmFile) {
  const code = Buffer.isBuffer(wasmFile) ? wasmFile : readBin(wasmFile);
  let instance;
  let errStr = '';
  const getMessage = () => {
    let msg = '';
    let c = instance.exports.getMessageChar();
    while (c !== 0) {
      msg += String.fromCharCode(c);
      c = instance.exports.getMessageChar();
    }
    return msg;
  };
  const errors = ['', 'Signal not found.', 'Too many signals set.', 'Signal already set.', 'Assert Failed.',
    'Not enough memory.', 'Input signal array access exceeds the size.'];
  const mod = await WebAssembly.compile(code);
  instance = await WebAssembly.instantiate(mod, {
    runtime: {
      exceptionHandler: (c) => { throw new Error((errors[c] || 'Unknown error.') + '\n' + errStr); },
      printErrorMessage: () => { errStr += getMessage() + '\n'; },
      writeBufferMessage: () => { getMessage(); },
      showSharedRWMemory: () => {},
    },
  });
  const ex = instance.exports;
  const n32 = ex.getFieldNumLen32();
  ex.getRawPrime();
  let prime = BigInt(0);
  for (let j = n32 - 1; j >= 0; j--) prime = (prime << BigInt(32)) | BigInt(ex.readSharedRWMemory(j) >>> 0);
  const witnessSize = ex.getWitnessSize();
  ex.init(0);
  let counter = 0;
  for (const k of Object.keys(input)) {
    const h = fnvHash(k);
    const hMSB = parseInt(h.slice(0, 8), 16);
    const hLSB = parseInt(h.slice(8, 16), 16);
    const vals = flatArray(input[k]);
    const size = ex.getInputSignalSize(hMSB, hLSB);
    if (size < 0) throw new Error(`Signal ${k} not found\n`);
    if (vals.length < size) throw new Error(`Not enough values for input signal ${k}\n`);
    if (vals.length > size) throw new Error(`Too many values for input signal ${k}\n`);
    for (let i = 0; i < vals.length; i++) {
      let v = BigInt(vals[i]) % prime;
      if (v < BigInt(0)) v += prime;
      for (let j = 0; j < n32; j++) {
        ex.writeSharedRWMemory(j, Number(v & BigInt(0xffffffff)));
        v >>= BigInt(32);
      }
      ex.setInputSignal(hMSB, hLSB, i);
      counter++;
    }
  }
  if (ex.getInputSize && counter < ex.getInputSize()) {
    throw new Error(`Not all inputs have been set. Only ${counter} out of ${ex.getInputSize()}`);
  }
  const n8 = n32 * 4;
  const out = Buffer.alloc(12 + 12 + 4 + n8 + 4 + 12 + witnessSize * n8);
  let o = 0;
  out.write('wtns', 0, 'latin1'); o = 4;
  out.writeUInt32LE(2, o); o += 4;
  out.writeUInt32LE(2, o); o += 4;
  out.writeUInt32LE(1, o); o += 4;
  out.writeUInt32LE(8 + n8, o); out.writeUInt32LE(0, o + 4); o += 8;
  out.writeUInt32LE(n8, o); o += 4;
  ex.getRawPrime();
  for (let j = 0; j < n32; j++) { out.writeUInt32LE(ex.readSharedRWMemory(j) >>> 0, o); o += 4; }
  out.writeUInt32LE(witnessSize, o); o += 4;
  out.writeUInt32LE(2, o); o += 4;
  const s2 = witnessSize * n8;
  out.writeUInt32LE(s2 % 0x100000000, o); out.writeUInt32LE(Math.floor(s2 / 0x100000000), o + 4); o += 8;
  for (let i = 0; i < witnessSize; i++) {
    ex.getWitness(i);
    for (let j = 0; j < n32; j++) { out.writeUInt32LE(ex.readSharedRWMemory(j) >>> 0, o); o += 4; }
  }
  return out;
}

// ---------------------------------------------------------------------------
// Witness calculation on the GPU from a witness program (nzcb/circuit.py write_program:
// nzcp_live = NZCPPubIdentity(1, 351, 0, 4, 2, 4) compiled by nzcb/nzcpgen.py), the
// MI355X replacement of the circom wasm for circuits this build compiles. The program
// carries the main's input names and sizes; inputs are mapped by name, as circom does.
// ---------------------------------------------------------------------------
function programInputs(prog) {
  const u32 = (o) => prog.readUInt32LE(o);
  const nc = u32(24), nt = u32(28), no = u32(32), nlev = u32(36);
  let o = 40 + nc * 32 + nt * 8 + no * 32 + (2 * nlev + 1) * 4;
  const n = u32(o); o += 4;
  const names = [];
  for (let i = 0; i < n; i++) {
    const len = u32(o); o += 4;
    const name = prog.toString('utf8', o, o + len); o += len;
    names.push([name, u32(o)]); o += 4;
  }
  // a remapped program (wtns.remapProgram) writes witnesses of its wire map's length
  const mapped = o + 8 <= prog.length && prog.toString('latin1', o, o + 4) === 'wmap';
  return { nWires: mapped ? u32(o + 4) : u32(8), names };
}

// nzcb_wprog_remap: a witness program re-indexed to the wire order of another .sym (e.g.
// circom's nzcp_live.sym, whose zkey expects circom's order), matching signals by name
// against the program's own .sym. Arguments: Buffers or file names.
function remapProgram(program, ownSym, targetSym) {
  return addon.remapWitnessProgram(readBin(program), readBin(ownSym), readBin(targetSym));
}

// fullProve's program argument: a path is read again only when its size or mtime changes (a
// server passes the same path on every call)
const programFiles = new Map();
function readProgram(x) {
  if (typeof x !== 'string') return readBin(x);
  const st = fs.statSync(x);
  const f = programFiles.get(x);
  if (f && f.size === st.size && f.mtimeMs === st.mtimeMs) return f.buf;
  const buf = fs.readFileSync(x);
  programFiles.set(x, { size: st.size, mtimeMs: st.mtimeMs, buf });
  return buf;
}

// loaded programs by content hash; a Buffer seen before skips the hash (a program of
// nzcp_live's size takes tens of ms to hash: per call, that was the Node path's bottleneck)
const programs = new Map();
const programsByBuf = new WeakMap();
function programFor(progBuf, device) {
  let byDev = programsByBuf.get(progBuf);
  const probe = probeOf(progBuf);
  if (byDev && byDev.probe !== probe) byDev = null;  // the Buffer now holds other contents
  if (byDev && byDev.has(device)) return byDev.get(device);
  const key = contentHash(progBuf) + ':' + device;
  let p = programs.get(key);
  if (!p) {
    p = { handle: addon.createWitnessProgram(progBuf, device), meta: programInputs(progBuf) };
    programs.set(key, p);
  }
  if (!byDev) {
    programsByBuf.set(progBuf, (byDev = new Map()));
    byDev.probe = probe;
  }
  byDev.set(device, p);
  return p;
}

// one signal value -> 32-byte LE at buf[off] (buf zero-filled): small non-negative numbers
// directly, everything else reduced mod r and written as four 64-bit words
const M64 = (BigInt(1) << BigInt(64)) - BigInt(1);
const B64 = BigInt(64);
function putSignal(buf, off, x) {
  if (typeof x === 'number' && Number.isSafeInteger(x) && x >= 0) {
    buf.writeUIntLE(x % 0x1000000000000, off, 6);
    if (x >= 0x1000000000000) buf.writeUInt16LE(Math.floor(x / 0x1000000000000), off + 6);
    return;
  }
  let v = BigInt(x) % R;
  if (v < BigInt(0)) v += R;
  for (let j = 0; j < 4; j++) { buf.writeBigUInt64LE(v & M64, off + 8 * j); v >>= B64; }
}

// the main's input object -> n_inputs x 32-byte LE values, by the program's input names
function programInputBuffer(input, meta) {
  const vals = [];
  for (const [name, size] of meta.names) {
    if (!(name in input)) throw new Error(`Signal ${name} not found\n`);
    const flat = flatArray(input[name]);
    if (flat.length < size) throw new Error(`Not enough values for input signal ${name}\n`);
    if (flat.length > size) throw new Error(`Too many values for input signal ${name}\n`);
    vals.push(...flat);
  }
  for (const k of Object.keys(input)) {
    if (!meta.names.some(([n]) => n === k)) throw new Error(`Signal ${k} not found\n`);
  }
  const buf = Buffer.alloc(32 * vals.length);
  vals.forEach((x, i) => putSignal(buf, 32 * i, x));
  return buf;
}

async function wtnsCalculateGpu(input, progBuf, device) {
  const { handle, meta } = programFor(progBuf, device);
  const buf = programInputBuffer(input, meta);
  const wit = await addon.calculateWitness(handle, buf);
  const hdr = Buffer.alloc(12 + 12 + 4 + 32 + 4 + 12);
  let o = 0;
  hdr.write('wtns', 0, 'latin1'); o = 4;
  hdr.writeUInt32LE(2, o); o += 4;
  hdr.writeUInt32LE(2, o); o += 4;
  hdr.writeUInt32LE(1, o); o += 4;
  hdr.writeUInt32LE(40, o); hdr.writeUInt32LE(0, o + 4); o += 8;
  hdr.writeUInt32LE(32, o); o += 4;
  let r = R;
  for (let j = 0; j < 32; j++) { hdr[o + j] = Number(r & BigInt(255)); r >>= BigInt(8); }
  o += 32;
  hdr.writeUInt32LE(meta.nWires, o); o += 4;
  hdr.writeUInt32LE(2, o); o += 4;
  hdr.writeUInt32LE(wit.length % 0x100000000, o); hdr.writeUInt32LE(Math.floor(wit.length / 0x100000000), o + 4);
  return Buffer.concat([hdr, wit]);
}

// wasmFile: a circom 2.0.x witness .wasm (run on the host CPU, as snarkjs does) or a
// witness program ("nzwp", run on the GPU). With a witness program the witness never
// leaves HBM: the program writes it into a device buffer that the proof reads
// (addon.fullProveDevice); only the input signals go up and the proof comes back.
async function fullProve(input, wasmFile, zkeyFileName, logger, options) {
  options = options || {};
  const code = readProgram(wasmFile);
  const device = options.device || 0;
  if (code.slice(0, 4).toString('latin1') === 'nzwp') {
    const { handle, meta } = programFor(code, device);
    const ctx = contextFor(zkeyFileName, device, options.lanes);
    const res = await addon.fullProveDevice(ctx, handle, programInputBuffer(input, meta), blindingFor(options),
      loggerFn(logger));
    return { proof: JSON.parse(res.proof), publicSignals: JSON.parse(res.publicSignals) };
  }
  const wtns = await wtnsCalculate(input, code);
  return prove(zkeyFileName, { type: 'mem', data: wtns }, logger, options);
}

// ---------------------------------------------------------------------------
// Verification key, verifier, Solidity calldata (SURVEY.md §8f ranks 1 and 4):
// snarkjs zKey.exportVerificationKey / plonk.verify / plonk.exportSolidityCallData.
// ---------------------------------------------------------------------------
const PROOF_POINTS = ['A', 'B', 'C', 'Z', 'T1', 'T2', 'T3', 'Wxi', 'Wxiw'];
const PROOF_EVALS = ['eval_a', 'eval_b', 'eval_c', 'eval_s1', 'eval_s2', 'eval_zw', 'eval_r'];
const VK_POINTS = ['Qm', 'Ql', 'Qr', 'Qo', 'Qc', 'S1', 'S2', 'S3'];

function le32(x) {
  let v = BigInt(x);
  const out = Buffer.alloc(32);
  for (let i = 0; i < 32; i++) { out[i] = Number(v & BigInt(255)); v >>= BigInt(8); }
  return out;
}
function g1Buf(p) { return String(p[2]) === '0' ? Buffer.alloc(64) : Buffer.concat([le32(p[0]), le32(p[1])]); }
function proofBuf(proof) {
  return Buffer.concat(PROOF_POINTS.map((k) => g1Buf(proof[k])).concat(PROOF_EVALS.map((k) => le32(proof[k]))));
}
function pubBuf(pub) { return Buffer.concat(pub.map(le32).concat([Buffer.alloc(0)])); }
function vkBuf(vk) {
  const head = Buffer.alloc(8);
  head.writeUInt32LE(Number(vk.nPublic), 0);
  head.writeUInt32LE(Number(vk.power), 4);
  const x2 = vk.X_2;
  return Buffer.concat([head, le32(vk.k1), le32(vk.k2)].concat(VK_POINTS.map((k) => g1Buf(vk[k])))
    .concat([le32(x2[0][0]), le32(x2[0][1]), le32(x2[1][0]), le32(x2[1][1]), le32(vk.w)]));
}

// snarkjs plonk.setup(r1csName, ptauName, zkeyName, logger) (snarkjs 0.4.12
// plonk_setup.js, run at /root/reference/Makefile:55,60): writes the PLONK zkey.
// Names may also be {type: "mem", data} objects; a {type: "mem"} zkeyName receives
// the bytes in .data.
async function setup(r1csName, ptauName, zkeyName, logger, options) {
  options = options || {};
  const log = loggerFn(logger);
  const zkey = addon.plonkSetup(readBin(r1csName), readBin(ptauName), options.device || 0);
  if (zkeyName && typeof zkeyName === 'object') zkeyName.data = new Uint8Array(zkey);
  else fs.writeFileSync(zkeyName, zkey);
  if (log) log(`Plonk setup: zkey of ${zkey.length} bytes`);
  return 0;
}

// binary verification key of a zkey: a file name is memory-mapped by the library
// (nzcb_vk_from_zkey_file), so nzcp_live's ~3.9 GB zkey is never read into a Buffer
// (fs.readFileSync refuses files past 2 GiB)
function vkOf(zkey) {
  return typeof zkey === 'string' ? addon.vkFromZkeyFile(zkey) : addon.vkFromZkey(readBin(zkey));
}

// the protocol id of a zkey (section 1: 1 = groth16, 2 = plonk), read through its section table;
// 0 for anything that is no zkey
function zkeyProtocol(zkey) {
  const fd = typeof zkey === 'string' ? fs.openSync(zkey, 'r') : null;
  const bytes = fd === null ? readBin(zkey) : null;
  const read = (pos, len) => {
    const b = Buffer.alloc(len);
    if (fd === null) return bytes.copy(b, 0, pos, pos + len) === len ? b : null;
    return fs.readSync(fd, b, 0, len, pos) === len ? b : null;
  };
  try {
    const head = read(0, 12);
    if (!head || head.toString('latin1', 0, 4) !== 'zkey') return 0;
    let pos = 12;
    for (let i = head.readUInt32LE(8); i > 0; i--) {
      const entry = read(pos, 12);
      if (!entry) return 0;
      if (entry.readUInt32LE(0) === 1) {
        const id = read(pos + 12, 4);
        return id ? id.readUInt32LE(0) : 0;
      }
      pos += 12 + Number(entry.readBigUInt64LE(4));
    }
    return 0;
  } finally {
    if (fd !== null) fs.closeSync(fd);
  }
}

// snarkjs zKey.exportVerificationKey: by the key's protocol id, the PLONK object or, for a Groth16
// key (id 1), {protocol: "groth16", curve, nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2,
// IC}. snarkjs's vk_alphabeta_12 is left out: its Fq12 layout cannot be pinned here, and neither
// snarkjs's verifier nor its Solidity template reads it.
async function exportVerificationKey(zkeyFileName) {
  if (zkeyProtocol(zkeyFileName) === 1) {
    return JSON.parse(addon.groth16Vk(typeof zkeyFileName === 'string' ? zkeyFileName : readBin(zkeyFileName)));
  }
  return JSON.parse(addon.vkToJson(vkOf(zkeyFileName)));
}

// snarkjs's `phase2` recipe for Groth16 (include/nzcb.h nzcb_groth16_setup,
// nzcb_groth16_contribute), with snarkjs's names and argument order, file names only; each runs on
// a worker thread. NZCB_DEVICE selects the GPU (-1 = on the host) when options.device is not given.
// zKey.newZKey(r1csName, ptauName, zkeyName, logger): the Groth16 proving key of the circuit from
//   a powers-of-tau file prepared for phase 2. A FRESH KEY HAS delta = 1: anyone can forge proofs
//   under it until zKey.contribute has run. No circuit hash is written and the bytes' parity with
//   snarkjs is unpinned.
// zKey.contribute(oldZkeyName, newZkeyName, name, entropy, logger): multiplies a fresh secret from
//   the OS CSPRNG, mixed with `entropy`, into delta. NO contribution record is written (`name` is
//   only logged), so `snarkjs zkey verify` does not accept the result.
async function newZKey(r1csName, ptauName, zkeyName, logger, options) {
  if (typeof r1csName !== 'string' || typeof ptauName !== 'string' || typeof zkeyName !== 'string') {
    throw new TypeError('newZKey: file names must be strings');
  }
  await addon.groth16Op(0, r1csName, ptauName, zkeyName, '', ptauDevice(options));
  const log = ptauLog(logger);
  if (log) {
    log('groth16 setup: key written with delta = 1 (contribute before use); NO circuit hash written ' +
        '(snarkjs zkey verify will not accept this file)');
  }
}
async function zkeyContribute(oldZkeyName, newZkeyName, name, entropy, logger, options) {
  if (typeof oldZkeyName !== 'string' || typeof newZkeyName !== 'string') {
    throw new TypeError('contribute: file names must be strings');
  }
  await addon.groth16Op(1, oldZkeyName, '', newZkeyName, entropy === undefined || entropy === null ? '' : String(entropy),
                        ptauDevice(options));
  const log = ptauLog(logger);
  if (log) {
    log(`zkey contribute: "${name || ''}" applied (the name is not recorded); NO contribution record written ` +
        '(snarkjs zkey verify will not accept this file)');
  }
}

// snarkjs zKey.exportSolidityVerifier(zkeyName, templates, logger) (`zkey export
// solidityverifier`, /root/reference/Makefile:57,62): the verifier contract's source.
// The snarkjs templates argument is not used (the contract is rendered by the library);
// options.name sets the contract name (the reference's deploy-script.js asks for "Verifier").
async function exportSolidityVerifier(zkeyFileName, templates, logger, options) {
  options = options || {};
  if (zkeyProtocol(zkeyFileName) === 1) throw new Error('groth16: the Solidity verifier is not implemented');
  const tp = options.transcriptPublic === undefined ? true : !!options.transcriptPublic;
  const src = addon.vkToSolidity(vkOf(zkeyFileName), options.name || 'PlonkVerifier', tp);
  const log = loggerFn(logger);
  if (log) log(`Solidity verifier: ${src.length} bytes`);
  return src;
}

async function verify(vkVerifier, publicSignals, proof, logger, options) {
  options = options || {};
  const tp = options.transcriptPublic === undefined ? true : !!options.transcriptPublic;
  const ok = addon.verify(vkBuf(vkVerifier), proofBuf(proof), pubBuf(publicSignals), tp);
  const log = loggerFn(logger);
  if (log) log(ok ? 'OK!' : 'Invalid proof');
  return ok;
}

// plonk.verify for many proofs of one key (include/nzcb.h nzcb_verify_batch): one pairing
// check for the batch and the G1 scalar multiplications on the GPU, on a worker thread (the
// event loop is not blocked). options: {device (default 0; -1 = on the host), transcriptPublic}.
// Resolves to one boolean per proof.
async function verifyBatch(vkVerifier, publicSignalsArray, proofArray, logger, options) {
  options = options || {};
  const tp = options.transcriptPublic === undefined ? true : !!options.transcriptPublic;
  const count = proofArray.length;
  if (publicSignalsArray.length !== count) throw new Error('verifyBatch: one publicSignals array per proof');
  const nPublic = count ? publicSignalsArray[0].length : 0;
  if (publicSignalsArray.some((p) => p.length !== nPublic)) {
    throw new Error('verifyBatch: every item has the same number of public signals');
  }
  const ok = await addon.verifyBatch(vkBuf(vkVerifier), Buffer.concat(proofArray.map(proofBuf).concat([Buffer.alloc(0)])),
    Buffer.concat(publicSignalsArray.map(pubBuf).concat([Buffer.alloc(0)])), count, tp,
    options.device === undefined ? 0 : options.device);
  const log = loggerFn(logger);
  if (log) log(`verifyBatch: ${ok.filter((x) => x).length} of ${count} valid`);
  return ok;
}

// snarkjs wtns.check(r1csFileName, wtnsFileName, logger) (`snarkjs wtns check`): does the
// witness satisfy every constraint of the r1cs? On the GPU (include/nzcb.h nzcb_r1cs_check), on
// a worker thread. Resolves to true / false and logs snarkjs's lines: "WITNESS IS CORRECT", or
// "WITNESS CHECKING FAILED" and one line per listed failing constraint. options: {device
// (default 0; -1 = on the host), badCap (how many failing constraints to list, default 8)}.
function warnFn(logger) {
  if (logger && typeof logger.warn === 'function') return (m) => logger.warn(m);
  return loggerFn(logger);
}
async function wtnsCheck(r1csFileName, wtnsFileName, logger, options) {
  options = options || {};
  const log = loggerFn(logger);
  const info = logger && typeof logger.info === 'function' ? (m) => logger.info(m) : log;
  const warn = warnFn(logger);
  const r1cs = typeof r1csFileName === 'string' ? r1csFileName : readBin(r1csFileName);
  const res = await addon.wtnsCheck(r1cs, readBin(wtnsFileName), options.device === undefined ? 0 : options.device,
    options.badCap === undefined ? 8 : options.badCap);
  if (res.nBad === 0) {
    if (info) info('WITNESS IS CORRECT');
    return true;
  }
  if (warn) {
    warn('WITNESS CHECKING FAILED');
    for (const k of res.bad) warn(`constraint ${k} is not satisfied`);
    if (res.nBad > res.bad.length) warn(`${res.nBad} constraints are not satisfied`);
  }
  return false;
}

// Key material examined on the GPU before use (include/nzcb.h nzcb_ptau_check, nzcb_zkey_check),
// on a worker thread; a file name is memory-mapped, a Buffer is copied. The names are `check`,
// not `verify`: snarkjs's `powersoftau verify` audits the ceremony's contributions, and this
// does not.
// powersOfTau.check(ptau, logger, {device (default 0; -1 = on the host), power}): every tauG1 point
// on the curve, P_0 the generator and P_i = tau P_(i-1) against the file's [tau]G2. With `power`
// only the 2^power + 6 points a circuit of that domain uses. Resolves to the finding
// {status: 'OK' | 'G2' | 'RANGE' | 'CURVE' | 'GENERATOR' | 'SEQUENCE', index, nBad, checked,
// pairingChecks} and logs one line.
function findingLine(name, f) {
  if (f.status === 'OK') return `${name}: OK (${f.checked} checked)`;
  const bad = f.nBad ? `, ${f.nBad} defective` : '';
  return `${name}: ${f.status} at ${f.index}${bad}`;
}
function keyFile(f) {
  return typeof f === 'string' ? f : readBin(f);
}
async function powersOfTauCheck(ptau, logger, options) {
  options = options || {};
  const info = logger && typeof logger.info === 'function' ? (m) => logger.info(m) : loggerFn(logger);
  const count = options.power === undefined ? 0 : Math.pow(2, options.power) + 6;
  const f = await addon.keyCheck(0, keyFile(ptau), options.device === undefined ? 0 : options.device, count);
  if (info) info(findingLine('tauG1', f));
  return f;
}
// snarkjs's `phase1` recipe (include/nzcb.h nzcb_ptau_new, nzcb_ptau_contribute,
// nzcb_ptau_prepare_phase2), with snarkjs's names and argument order, file names only; each runs
// on a worker thread. NZCB_DEVICE selects the GPU (-1 = on the host) when options.device is not
// given.
// powersOfTau.newAccumulator(curve, power, fileName, logger): curve is "bn128" or an object whose
//   name is that.
// powersOfTau.contribute(oldPtauFileName, newPtauFileName, name, entropy, logger): multiplies
//   fresh secrets from the OS CSPRNG, mixed with `entropy`, into every section. NO contribution
//   record is written (`name` is only logged), so `snarkjs powersoftau verify` does not accept the
//   result: this re-randomises a file for yourself, it is not an audited ceremony.
// powersOfTau.preparePhase2(oldPtauFileName, newPtauFileName, logger): appends the Lagrange
//   sections 12-15 that snarkjs's setups read.
function ptauDevice(options) {
  if (options && options.device !== undefined) return options.device;
  return process.env.NZCB_DEVICE === undefined ? 0 : Number(process.env.NZCB_DEVICE);
}
function ptauLog(logger) {
  return logger && typeof logger.info === 'function' ? (m) => logger.info(m) : loggerFn(logger);
}
async function newAccumulator(curve, power, fileName, logger) {
  const curveName = curve && typeof curve === 'object' ? curve.name : curve;
  if (String(curveName).toLowerCase() !== 'bn128') throw new Error(`Curve not supported: ${curveName}`);
  if (typeof fileName !== 'string') throw new TypeError('newAccumulator: fileName must be a string');
  await addon.ptauOp(0, '', fileName, Number(power), '', 0);
  const log = ptauLog(logger);
  if (log) log(`powersoftau new: bn128, power ${power}, no contributions`);
}
async function contribute(oldPtauFileName, newPtauFileName, name, entropy, logger, options) {
  if (typeof oldPtauFileName !== 'string' || typeof newPtauFileName !== 'string') {
    throw new TypeError('contribute: file names must be strings');
  }
  await addon.ptauOp(1, oldPtauFileName, newPtauFileName, 0, entropy === undefined || entropy === null ? '' : String(entropy),
                     ptauDevice(options));
  const log = ptauLog(logger);
  if (log) {
    log(`powersoftau contribute: "${name || ''}" applied; NO contribution record written ` +
        '(snarkjs powersoftau verify will not accept this file)');
  }
}
async function preparePhase2(oldPtauFileName, newPtauFileName, logger, options) {
  if (typeof oldPtauFileName !== 'string' || typeof newPtauFileName !== 'string') {
    throw new TypeError('preparePhase2: file names must be strings');
  }
  await addon.ptauOp(2, oldPtauFileName, newPtauFileName, 0, '', ptauDevice(options));
  const log = ptauLog(logger);
  if (log) log('powersoftau prepare phase2: sections 12-15 written');
}

// zKey.check(zkey, logger, {device}): the key's cosets, its PTau against X_2, and per polynomial
// the canonical values, the evaluations against the coefficients and the header's commitment.
// Resolves to {ok, header, srs, parts: {Qm, ..., S3, L0, ...}} and logs one line per finding.
// Whether the key belongs to your circuit is not examined: that needs the r1cs.
async function zKeyCheck(zkey, logger, options) {
  options = options || {};
  const info = logger && typeof logger.info === 'function' ? (m) => logger.info(m) : loggerFn(logger);
  const r = await addon.keyCheck(1, keyFile(zkey), options.device === undefined ? 0 : options.device, 0);
  if (info) {
    info(findingLine('k1, k2', r.header));
    info(findingLine('PTau', r.srs));
    for (const name of Object.keys(r.parts)) info(findingLine(name, r.parts[name]));
  }
  return r;
}

// snarkjs r1cs.info(r1csFileName): the circuit's sizes (host only, no GPU)
async function r1csInfo(r1csFileName, logger) {
  const v = addon.r1csInfo(r1csFileName);
  const out = { nVars: v[0], nOutputs: v[1], nPubInputs: v[2], nPrvInputs: v[3], nConstraints: v[4] };
  const log = logger && typeof logger.info === 'function' ? (m) => logger.info(m) : loggerFn(logger);
  if (log) {
    log(`# of Wires: ${out.nVars}`);
    log(`# of Constraints: ${out.nConstraints}`);
    log(`# of Private Inputs: ${out.nPrvInputs}`);
    log(`# of Public Inputs: ${out.nPubInputs}`);
    log(`# of Outputs: ${out.nOutputs}`);
  }
  return out;
}

async function exportSolidityCallData(proof, publicSignals) {
  return addon.calldata(proofBuf(proof), pubBuf(publicSignals));
}

// nzcp witness on the GPU (include/nzcb.h nzcb_nzcp_witness): the NZCPPubIdentity
// public signals and semantic signals of one or more circuit inputs (the object
// plonk.fullProve takes, test/nzcp.js:41). Throws like calculateWitness when a pass
// fails one of the circuit's constraints.
const NZCP_PARAMS = { live: [1, 351, 0, 4], example: [0, 314, 0, 4] };
const NZCP_STATUS = ['ok', 'toBeSigned bit check', 'toBeSignedLen > MaxToBeSignedBytes',
  'LessThan operands out of range', 'QuinSelector index out of range', 'CBOR type is not a map',
  'CBOR map length > 23', 'CBOR type is not a string', 'negative toBeSignedLen (unpinned)'];
const NZCP_RECORD_BYTES = 288;

function fieldLE(v) {
  let x = BigInt(v) % R;
  if (x < BigInt(0)) x += R;
  return le32(x.toString());
}

function nzcpWitness(inputs, options) {
  options = options || {};
  const list = Array.isArray(inputs) ? inputs : [inputs];
  const params = options.params || NZCP_PARAMS[options.circuit || 'live'];
  const bufs = [];
  for (const inp of list) {
    if (inp.toBeSigned.length !== 8 * params[1] || inp.data.length !== 160) {
      throw new Error(`nzcp input: toBeSigned must have ${8 * params[1]} bits and data 160`);
    }
    for (const b of inp.toBeSigned) bufs.push(fieldLE(b));
    bufs.push(fieldLE(inp.toBeSignedLen));
    for (const b of inp.data) bufs.push(fieldLE(b));
  }
  const raw = addon.nzcpWitness(Buffer.concat(bufs), list.length, params, options.device || 0);
  const out = [];
  for (let i = 0; i < list.length; i++) {
    const r = raw.subarray(i * NZCP_RECORD_BYTES, (i + 1) * NZCP_RECORD_BYTES);
    const status = r.readInt32LE(0);
    if (status !== 0) {
      throw new Error(`Assert Failed (nzcp pass ${i}): ${NZCP_STATUS[status] || status} (detail ${r.readInt32LE(4)})`);
    }
    const nullifier = r.subarray(128, 192);
    out.push({
      publicSignals: [0, 1, 2].map((k) => BigInt('0x' + Buffer.from(r.subarray(192 + 32 * k, 224 + 32 * k))
        .reverse().toString('hex')).toString()),
      exp: r.readUInt32LE(8),
      vcPos: r.readInt32LE(12),
      nullifier: nullifier.subarray(0, Math.max(0, Math.min(64, r.readInt32LE(28)))).toString('latin1'),
      toBeSignedHash: r.subarray(32, 64).toString('hex'),
      nullifierHash: r.subarray(64, 128).toString('hex'),
    });
  }
  return Array.isArray(inputs) ? out : out[0];
}

// Pass signatures (include/nzcb.h nzcb_p256_*): COSE ES256 = ECDSA P-256 over the SHA-256 of the
// Sig_structure, what @vaxxnz/nzcp's verifyPassURIOffline checks in the reference's tests
// (test/nzcp.js:16) before a pass is used. options.key: {x, y} base64url as in a DID
// document's publicKeyJwk, a 64-byte Buffer x || y, or 'example' (nzcp.EXAMPLE_PUBLIC_KEY);
// whether a key is the issuer's is the caller's business. options.device: the GPU (default 0),
// -1 = the host path. options.now (seconds): adds expired / notYetValid. Resolves to one object
// per pass: {valid, status (0 ok, 1 invalid, 2 r or s out of range, null = not verified), reason,
// alg, kid, iss, nbf, exp}; a pass that is malformed, not ES256 or whose signature is not 64
// bytes is reported with its reason and not sent to the verifier.
const nzcpHost = require('./nzcp.js');
const SIG_REASON = [null, 'invalid signature', 'signature out of range'];

function b64url(s) {
  return Buffer.from(String(s).replace(/-/g, '+').replace(/_/g, '/'), 'base64');
}

function p256KeyBuffer(key) {
  if (key === 'example') key = nzcpHost.EXAMPLE_PUBLIC_KEY;
  if (Buffer.isBuffer(key) || key instanceof Uint8Array) {
    if (key.length !== 64) throw new Error('a P-256 public key is 32 + 32 bytes');
    return Buffer.from(key);
  }
  if (!key || key.x === undefined || key.y === undefined) {
    throw new Error("verifyPass needs options.key: {x, y}, a 64-byte Buffer or 'example'");
  }
  const x = b64url(key.x);
  const y = b64url(key.y);
  if (x.length !== 32 || y.length !== 32) throw new Error('a P-256 public key is 32 + 32 bytes');
  return Buffer.concat([x, y]);
}

// SHA-256 digests (32 bytes each) against r || s signatures (64 bytes each) -> status numbers
async function p256Verify(key, hashes, sigs, options) {
  options = options || {};
  return addon.p256Verify(p256KeyBuffer(key), Buffer.concat(hashes), Buffer.concat(sigs),
    options.device === undefined ? 0 : options.device);
}

// Pass decode (include/nzcb.h nzcb_nzcp_decode): URIs -> records, on the GPU (options.device,
// default 0) or on the host (-1), on a worker thread. options.circuit 'live' | 'example' adds
// `inputs`: one Buffer, pass i's input signals (32-byte LE each, what wtns.calculate's programs
// and nzcp.witness take) at i * (8 max + 161) * 32, zeros where the record's fits is 0;
// options.data: the 20 pass-through bytes, one Buffer for all passes or one per pass.
// Resolves to {records, inputs?}; a record's absent fields are null.
const PASS_STATUS = ['OK', 'LENGTH', 'PREFIX', 'BASE32', 'TRUNCATED', 'CBOR', 'NOT_COSE', 'HEADER', 'CLAIMS'];
const PASS_BYTES = 304;
{
  const lay = addon.nzcpPassLayout();
  if (lay[0] !== PASS_BYTES || lay[1] !== 208 || lay[2] !== 272) {
    throw new Error(`nzcb: nzcb_nzcp_pass is laid out as ${lay}, index.js expects 304,208,272`);
  }
}

function passRecord(r) {
  const present = r.readUInt32LE(12);
  const u64 = (off) => {
    const v = r.readBigUInt64LE(off);
    return v <= BigInt(Number.MAX_SAFE_INTEGER) ? Number(v) : v;
  };
  const first = (off, cap, len) => Buffer.from(r.subarray(off, off + Math.min(cap, len)));
  const status = r.readInt32LE(0);
  return {
    status,
    statusName: PASS_STATUS[status],
    detail: r.readUInt32LE(4),
    version: r.readUInt32LE(8),
    alg: present & 1 ? r.readInt32LE(16) : null,
    kid: present & 2 ? first(80, 32, r.readUInt32LE(20)).toString('utf8') : null,
    kidLen: r.readUInt32LE(20),
    iss: present & 4 ? first(144, 64, r.readUInt32LE(24)).toString('utf8') : null,
    issLen: r.readUInt32LE(24),
    nbf: present & 8 ? u64(64) : null,
    exp: present & 16 ? u64(72) : null,
    cti: present & 32 ? first(112, 32, r.readUInt32LE(28)) : null,
    ctiLen: r.readUInt32LE(28),
    sig: present & 64 ? first(208, 64, 64) : null,
    sigLen: r.readUInt32LE(32),
    coseLen: r.readUInt32LE(36),
    protectedOff: r.readUInt32LE(40),
    protectedLen: r.readUInt32LE(44),
    payloadOff: r.readUInt32LE(48),
    payloadLen: r.readUInt32LE(52),
    toBeSignedLen: r.readUInt32LE(56),
    fits: r.readUInt32LE(60) !== 0,
    toBeSignedHash: r.subarray(272, 304).toString('hex'),
  };
}

async function decodeRaw(uris, options, key) {
  const bufs = uris.map((u) => (Buffer.isBuffer(u) ? u : Buffer.from(String(u), 'utf8')));
  const offsets = Buffer.alloc(4 * (bufs.length + 1));
  let at = 0;
  bufs.forEach((b, i) => {
    at += b.length;
    if (at > 0x80000000) throw new Error('more than 2^31 bytes of URIs');
    offsets.writeUInt32LE(at, 4 * (i + 1));
  });
  let maxTbs = 0;
  if (options.circuit !== undefined) {
    if (!NZCP_PARAMS[options.circuit]) throw new Error("options.circuit is 'live' or 'example'");
    maxTbs = NZCP_PARAMS[options.circuit][1];
  }
  let data = null;
  if (options.data !== undefined && options.data !== null) {
    data = Array.isArray(options.data) ? Buffer.concat(options.data.map((d) => Buffer.from(d)))
      : Buffer.from(options.data);
    if (data.length === 20 && bufs.length !== 1) data = Buffer.concat(bufs.map(() => data));
    if (data.length !== 20 * bufs.length) throw new Error('data must be 20 bytes, or 20 bytes per pass');
  }
  const raw = await addon.nzcpDecode(Buffer.concat(bufs), offsets, maxTbs, data,
    options.device === undefined ? 0 : options.device, key || null);
  raw.passes = bufs.map((_, i) => passRecord(raw.records.subarray(i * PASS_BYTES, (i + 1) * PASS_BYTES)));
  return raw;
}

async function decodePasses(uris, options) {
  options = options || {};
  const raw = await decodeRaw(uris, options, null);
  const out = { records: raw.passes };
  if (raw.inputs) out.inputs = raw.inputs;
  return out;
}

// verifyPasses with options.decode = 'device': the URIs go to the library as they are, are decoded
// there (on options.device, or on the host with -1) and each record's digest is checked against
// its signature; no per-pass decoding or hashing in JavaScript. Same objects and reason texts as
// the default route, except "malformed pass: <status name> at <detail>"; a record keeps the
// first 32 bytes of a kid and 64 of an iss.
async function verifyPassesDecoded(uris, options) {
  const raw = await decodeRaw(uris, { device: options.device }, p256KeyBuffer(options.key));
  return raw.passes.map((r, i) => {
    const d = { valid: false, status: null, reason: null, alg: null, kid: null, iss: null, nbf: null, exp: null };
    if (r.status !== 0) {
      d.reason = `malformed pass: ${r.statusName} at ${r.detail}`;
      return d;
    }
    Object.assign(d, { alg: r.alg, kid: r.kid, iss: r.iss, nbf: r.nbf, exp: r.exp });
    if (options.now !== undefined) {
      d.expired = typeof d.exp === 'number' && options.now >= d.exp;
      d.notYetValid = typeof d.nbf === 'number' && options.now < d.nbf;
    }
    if (d.alg !== -7) {
      d.reason = `unsupported alg ${d.alg} (ES256 is -7)`;
    } else if (r.sig === null || r.sigLen !== 64) {
      d.reason = 'signature is not 64 bytes';
    } else {
      d.status = raw.status[i];
      d.valid = d.status === 0;
      d.reason = SIG_REASON[d.status];
    }
    return d;
  });
}

async function verifyPasses(uris, options) {
  options = options || {};
  if (options.decode !== undefined) {
    if (options.decode !== 'device') throw new Error("options.decode is 'device' or left out");
    return verifyPassesDecoded(uris, options);
  }
  const key = p256KeyBuffer(options.key);
  const out = [];
  const sent = [];
  const hashes = [];
  const sigs = [];
  for (const uri of uris) {
    const d = { valid: false, status: null, reason: null, alg: null, kid: null, iss: null, nbf: null, exp: null };
    out.push(d);
    let pass;
    try {
      pass = nzcpHost.decodePass(uri);
      Object.assign(d, nzcpHost.protectedHeader(uri));
      const [cwt] = nzcpHost.cborDecode(pass.payload, 0);
      Object.assign(d, { iss: cwt.get(1), nbf: cwt.get(5), exp: cwt.get(4) });
    } catch (e) {
      d.reason = `malformed pass: ${e.message}`;
      continue;
    }
    if (options.now !== undefined) {
      d.expired = typeof d.exp === 'number' && options.now >= d.exp;
      d.notYetValid = typeof d.nbf === 'number' && options.now < d.nbf;
    }
    if (d.alg !== -7) {
      d.reason = `unsupported alg ${d.alg} (ES256 is -7)`;
    } else if (!Buffer.isBuffer(pass.signature) || pass.signature.length !== 64) {
      d.reason = 'signature is not 64 bytes';
    } else {
      hashes.push(crypto.createHash('sha256').update(nzcpHost.toBeSigned(uri)).digest());
      sigs.push(pass.signature);
      sent.push(d);
    }
  }
  if (sent.length) {
    const st = await addon.p256Verify(key, Buffer.concat(hashes), Buffer.concat(sigs),
      options.device === undefined ? 0 : options.device);
    sent.forEach((d, i) => {
      d.status = st[i];
      d.valid = st[i] === 0;
      d.reason = SIG_REASON[st[i]];
    });
  }
  return out;
}

async function verifyPass(uri, options) {
  return (await verifyPasses([uri], options))[0];
}

module.exports = {
  plonk: { setup, prove, fullProve, verify, verifyBatch, exportSolidityCallData },
  zKey: { exportVerificationKey, exportSolidityVerifier, check: zKeyCheck, newZKey, contribute: zkeyContribute },
  powersOfTau: { check: powersOfTauCheck, newAccumulator, contribute, preparePhase2 },
  nzcp: Object.assign({}, nzcpHost, { witness: nzcpWitness, verifyPass, verifyPasses, p256Verify, decodePasses }),
  wtns: { calculate: wtnsCalculate, remapProgram, check: wtnsCheck },
  r1cs: { info: r1csInfo },
  version: addon.version,
  deviceCount: addon.deviceCount,
  _addon: addon,
  _programInputBuffer: programInputBuffer,  // tests: the input signals' 32-byte encoding
};
