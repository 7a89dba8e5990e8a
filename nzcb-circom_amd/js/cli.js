#!/usr/bin/env node
'use strict';
// `snarkjs plonk setup|prove|fullprove` equivalent on the MI355X prover (SURVEY.md §8b):
//   node cli.js plonk setup     <circuit.r1cs> <pot.ptau> <circuit.zkey>
//   node cli.js plonk prove     <circuit.zkey> <witness.wtns> <proof.json> <public.json>
//   node cli.js plonk fullprove <input.json> <circuit.wasm> <circuit.zkey> <proof.json> <public.json>
//   node cli.js plonk verify    <verification_key.json> <public.json> <proof.json>
//     (prints "OK!" and exits 0 for a valid proof, "Invalid proof" and exit code 1 otherwise,
//     as snarkjs's CLI verb; host only, no GPU)
// and `snarkjs zkey export verificationkey|solidityverifier|soliditycalldata` (Makefile:56-62):
//   node cli.js zkey export verificationkey <circuit.zkey> <verification_key.json>
//   node cli.js zkey export solidityverifier <circuit.zkey> <Verifier.sol> [contract name]
//   node cli.js zkey export soliditycalldata <public.json> <proof.json>
// and `snarkjs wtns check` / `snarkjs r1cs info`:
//   node cli.js wtns check <circuit.r1cs> <witness.wtns>
//     (prints "WITNESS IS CORRECT" and exits 0, or "WITNESS CHECKING FAILED" with the failing
//     constraints and exit code 1; NZCB_DEVICE=-1 checks on the host)
//   node cli.js r1cs info  <circuit.r1cs>
// and the key material examined before use (not snarkjs's `powersoftau verify`, which audits the
// ceremony's contributions):
//   node cli.js powersoftau check <pot.ptau> [power]
//   node cli.js zkey check <circuit.zkey>
//     (one line per finding; exit code 0 only when everything is OK; NZCB_DEVICE=-1 checks on the host)
// and the signature check of NZ COVID Passes (what verifyPassURIOffline does in the reference's tests):
//   node cli.js nzcp verify <file with one pass URI per line> [example | <x> <y>]
//     (the issuer's P-256 key as base64url JWK coordinates, default the specification's example
//     key; prints "OK", "INVALID SIGNATURE" or the reason per pass and exits 0 only if all are
//     valid; NZCB_DEVICE=-1 verifies on the host)
// and the `phase1` recipe of snarkjs (Makefile), with only the program name changed:
//   node cli.js powersoftau new bn128 <power> <pot_0000.ptau> -v
//   node cli.js powersoftau contribute <pot_0000.ptau> <pot_0001.ptau> --name="First contribution" -v
//   node cli.js powersoftau prepare phase2 <pot_0001.ptau> <pot_final.ptau> -v
//     (contribute draws its secrets from the OS, mixed with -e=<entropy>; it writes NO contribution
//     record, so `snarkjs powersoftau verify` does not accept the file; NZCB_DEVICE=-1 runs on the host)
// and the first three lines of the `phase2` recipe for Groth16, with only the program name changed:
//   node cli.js groth16 setup <circuit.r1cs> <pot_final.ptau> <circuit_0000.zkey> -v
//   node cli.js zkey contribute <circuit_0000.zkey> <circuit_0001.zkey> --name="1st Contributor Name" -v
//   node cli.js zkey export verificationkey <circuit_0001.zkey> <verification_key.json>
//     (a fresh key has delta = 1: anyone can forge proofs under it until it has been contributed
//     to. Setup writes NO circuit hash and contribute NO contribution record, so `snarkjs zkey
//     verify` does not accept the files, and their parity with snarkjs's bytes is unpinned. There is
//     no Groth16 prover, verifier or Solidity verifier here: `zkey export solidityverifier` on a
//     Groth16 key exits non-zero. NZCB_DEVICE=-1 runs on the host)
// Output JSON is written like snarkjs's CLI (stringifyBigInts, 1-space indent).
const fs = require('fs');
const nz = require('./index.js');

function usage() {
  console.error('usage: cli.js plonk setup <r1cs> <ptau> <zkey>\n' +
                '       cli.js plonk prove <zkey> <wtns> <proof.json> <public.json>\n' +
                '       cli.js plonk fullprove <input.json> <wasm> <zkey> <proof.json> <public.json>\n' +
                '       cli.js plonk verify <verification_key.json> <public.json> <proof.json>\n' +
                '       cli.js zkey export verificationkey <zkey> <verification_key.json>\n' +
                '       cli.js zkey export solidityverifier <zkey> <verifier.sol> [contract name]\n' +
                '       cli.js zkey export soliditycalldata <public.json> <proof.json>\n' +
                '       cli.js wtns check <r1cs> <wtns>\n' +
                '       cli.js powersoftau check <ptau> [power]\n' +
                '       cli.js zkey check <zkey>\n' +
                '       cli.js r1cs info <r1cs>\n' +
                '       cli.js nzcp verify <file with one pass URI per line> [example | <x> <y>]\n' +
                '       cli.js powersoftau new bn128 <power> <new.ptau> [-v]\n' +
                '       cli.js powersoftau contribute <old.ptau> <new.ptau> [--name=<text>] [-e=<entropy>] [-v]\n' +
                '       cli.js powersoftau prepare phase2 <old.ptau> <new.ptau> [-v]\n' +
                '       cli.js groth16 setup <r1cs> <ptau> <zkey> [-v]\n' +
                '       cli.js zkey contribute <old.zkey> <new.zkey> [--name=<text>] [-e=<entropy>] [-v]\n' +
                '         (groth16 setup writes a key with delta = 1: contribute before use. NO circuit hash and NO\n' +
                '         contribution record are written: snarkjs zkey verify does not accept these files. There is\n' +
                '         no Groth16 prover, verifier or Solidity verifier here.)');
  process.exit(1);
}

async function zkeyExport(argv) {
  if (argv[1] !== 'export') usage();
  if (argv[2] === 'verificationkey' && argv.length === 5) {
    const vk = await nz.zKey.exportVerificationKey(argv[3]);
    fs.writeFileSync(argv[4], JSON.stringify(vk, null, 1), 'utf-8');
  } else if (argv[2] === 'solidityverifier' && (argv.length === 5 || argv.length === 6)) {
    const src = await nz.zKey.exportSolidityVerifier(argv[3], null, null, { name: argv[5] });
    fs.writeFileSync(argv[4], src, 'utf-8');
  } else if (argv[2] === 'soliditycalldata' && argv.length === 5) {
    const pub = JSON.parse(fs.readFileSync(argv[3], 'utf8'));
    const proof = JSON.parse(fs.readFileSync(argv[4], 'utf8'));
    console.log(await nz.plonk.exportSolidityCallData(proof, pub));
  } else {
    usage();
  }
}

async function keyCheck(argv) {
  const say = { info: (m) => console.log(m) };
  const device = process.env.NZCB_DEVICE === undefined ? 0 : Number(process.env.NZCB_DEVICE);
  if (argv[0] === 'zkey') {
    const r = await nz.zKey.check(argv[2], say, { device });
    process.exit(r.ok ? 0 : 1);
  }
  const power = argv.length === 4 ? Number(argv[3]) : undefined;
  if (power !== undefined && !(Number.isInteger(power) && power >= 0 && power <= 28)) usage();
  const f = await nz.powersOfTau.check(argv[2], say, { device, power });
  process.exit(f.status === 'OK' ? 0 : 1);
}

// powersoftau new | contribute | prepare phase2 with snarkjs's options: -v (log to the console),
// --name=<text> / -n=<text> and --entropy=<text> / -e=<text> (contribute)
async function phase1(argv) {
  const opts = { name: '', entropy: '' };
  const args = [];
  let verbose = false;
  for (const a of argv.slice(1)) {
    const m = /^(--name|-n|--entropy|-e)=(.*)$/s.exec(a);
    if (m) opts[m[1] === '--name' || m[1] === '-n' ? 'name' : 'entropy'] = m[2];
    else if (a === '-v' || a === '--verbose') verbose = true;
    else if (a.startsWith('-')) usage();
    else args.push(a);
  }
  const logger = verbose ? { info: (m) => console.log(m) } : null;
  if (args[0] === 'new' && args.length === 4) {
    const power = Number(args[2]);
    if (!Number.isInteger(power)) usage();
    return nz.powersOfTau.newAccumulator(args[1], power, args[3], logger);
  }
  if (args[0] === 'contribute' && args.length === 3) {
    // the CLI always says what the file is not, -v or not
    const say = { info: (m) => console.log(m) };
    return nz.powersOfTau.contribute(args[1], args[2], opts.name, opts.entropy, say);
  }
  if (args[0] === 'prepare' && args[1] === 'phase2' && args.length === 4) {
    return nz.powersOfTau.preparePhase2(args[2], args[3], logger);
  }
  usage();
}

// groth16 setup | zkey contribute with the same options
async function phase2(argv) {
  const opts = { name: '', entropy: '' };
  const args = [];
  for (const a of argv.slice(1)) {
    const m = /^(--name|-n|--entropy|-e)=(.*)$/s.exec(a);
    if (m) opts[m[1] === '--name' || m[1] === '-n' ? 'name' : 'entropy'] = m[2];
    else if (a === '-v' || a === '--verbose') continue;
    else if (a.startsWith('-')) usage();
    else args.push(a);
  }
  // the CLI always says what the file is not, -v or not
  const say = { info: (m) => console.log(m) };
  if (argv[0] === 'groth16' && args[0] === 'setup' && args.length === 4) {
    return nz.zKey.newZKey(args[1], args[2], args[3], say);
  }
  if (argv[0] === 'zkey' && args[0] === 'contribute' && args.length === 3) {
    return nz.zKey.contribute(args[1], args[2], opts.name, opts.entropy, say);
  }
  usage();
}

async function main(argv) {
  if (argv[0] === 'powersoftau' && (argv[1] === 'new' || argv[1] === 'contribute' || argv[1] === 'prepare')) return phase1(argv);
  if (argv[0] === 'groth16' || (argv[0] === 'zkey' && argv[1] === 'contribute')) return phase2(argv);
  if (argv[0] === 'zkey' && argv[1] === 'check' && argv.length === 3) return keyCheck(argv);
  if (argv[0] === 'powersoftau' && argv[1] === 'check' && (argv.length === 3 || argv.length === 4)) return keyCheck(argv);
  if (argv[0] === 'zkey') return zkeyExport(argv);
  if (argv[0] === 'wtns' && argv[1] === 'check' && argv.length === 4) {
    const say = { info: (m) => console.log(m), warn: (m) => console.log(m), debug: () => {} };
    const device = process.env.NZCB_DEVICE === undefined ? 0 : Number(process.env.NZCB_DEVICE);
    const ok = await nz.wtns.check(argv[2], argv[3], say, { device });
    process.exit(ok ? 0 : 1);
  }
  if (argv[0] === 'r1cs' && argv[1] === 'info' && argv.length === 3) {
    await nz.r1cs.info(argv[2], { info: (m) => console.log(m) });
    return;
  }
  if (argv[0] === 'nzcp' && argv[1] === 'verify' && (argv.length === 3 || argv.length === 4 || argv.length === 5)) {
    if (argv.length === 4 && argv[3] !== 'example') usage();
    const key = argv.length === 5 ? { x: argv[3], y: argv[4] } : 'example';
    const device = process.env.NZCB_DEVICE === undefined ? 0 : Number(process.env.NZCB_DEVICE);
    const uris = fs.readFileSync(argv[2], 'utf8').split(/\r?\n/).map((l) => l.trim()).filter((l) => l);
    const res = await nz.nzcp.verifyPasses(uris, { key, device });
    for (const r of res) console.log(r.valid ? 'OK' : (r.status === 1 ? 'INVALID SIGNATURE' : r.reason));
    process.exit(res.length && res.every((r) => r.valid) ? 0 : 1);
  }
  if (argv[0] !== 'plonk') usage();
  const logger = process.env.NZCB_VERBOSE ? { debug: (m) => console.error(m) } : null;
  let res, out;
  if (argv[1] === 'setup' && argv.length === 5) {
    await nz.plonk.setup(argv[2], argv[3], argv[4], logger);
    return;
  }
  if (argv[1] === 'verify' && argv.length === 5) {
    const vk = JSON.parse(fs.readFileSync(argv[2], 'utf8'));
    const pub = JSON.parse(fs.readFileSync(argv[3], 'utf8'));
    const proof = JSON.parse(fs.readFileSync(argv[4], 'utf8'));
    const ok = await nz.plonk.verify(vk, pub, proof, logger);
    console.log(ok ? 'OK!' : 'Invalid proof');
    process.exit(ok ? 0 : 1);
  }
  if (argv[1] === 'prove' && argv.length === 6) {
    res = await nz.plonk.prove(argv[2], argv[3], logger);
    out = argv.slice(4);
  } else if (argv[1] === 'fullprove' && argv.length === 7) {
    const input = JSON.parse(fs.readFileSync(argv[2], 'utf8'));
    res = await nz.plonk.fullProve(input, argv[3], argv[4], logger);
    out = argv.slice(5);
  } else {
    usage();
  }
  fs.writeFileSync(out[0], JSON.stringify(res.proof, null, 1), 'utf-8');
  fs.writeFileSync(out[1], JSON.stringify(res.publicSignals, null, 1), 'utf-8');
}

main(process.argv.slice(2)).then(() => process.exit(0), (e) => {
  console.error(e && e.message ? e.message : e);
  process.exit(1);
});
