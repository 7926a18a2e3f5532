// clean_adapter -- the clean_illumina module's adapter trimmer (clean_illumina/clean_adapter.cpp) with every alignment made on the
// GPU (CLEAN section of include/dbgk.h).  Same command line, same two output files: the cleaned reads (gzip) and the statistics.
// -t sizes nothing on the device.  The default adapter files (-a Both-adapter | R1-adapter | R2-adapter) are looked for in the
// directory DBGK_ADAPTER_DIR names, then at the reference's own path.
#include "clean_common.h"

static int Alignment_score_cutoff = 12;
static int Minimum_trimmed_read_len = 75;
static int Also_use_adapterRC = 0;
static string illumina_adapter_file = "Both-adapter";
static int threadNum = 3;

static void usage()
{
	cout << "Description:\nclean_adapter identifies and trims adapter sequence in raw reads by ungapped local dynamic programming alignment. "
	        "The program loads adapter sequences as aligning target from a default self-taken or specially user-defined multiple-fasta format "
	        "file by parameter (-a), in which more records can be given at the same time.  In theory, this program can be used to filter any "
	        "contaminant sequences besides adapters, however, this version is specifically written for trimming adapter, which considers "
	        "adapters locating on the tail part of reads, moreover, the alignment search will stop when find the first qualified hit "
	        "(>=minimum alignment score) for each reads. The alignment algorithm used ungapped dynamic programming local alignment, with a "
	        "score matrix [match:1; mismatch:-2], and reports only the best hit, and the aligning score cutoff can be set by a parameter (-s). "
	        "The program runs in a multiple thread mode (-t). The input file should be fastq or gzip-fastq format, and there are two resulting "
	        "files: one is the clean reads file, and the other one is a statistics file.\n";
	cout << "\nUsage:\n  clean_adapter  <Input.fq.gz> <Output.clean.gz> <Output.clean.stat> " << endl;
	cout << "   Author: Fanwei, fanweiagis@126.com" << endl;
	cout << "   Version 1.1;" << endl;
	cout << "   -a <str>   contaminant sequence file: Both-adapter, R1-adapter, R2-adapter for default adapter files, otherwise for "
	        "user-defined cotaminant file, default=" << illumina_adapter_file << endl;
	cout << "   -b <int>   use both strands of sequence for alignment, 0: no; 1:yes; default=" << Also_use_adapterRC << endl;
	cout << "   -s <int>   minimum alignment score, score matrix [match:1; mismatch:-2],default=" << Alignment_score_cutoff << endl;
	cout << "   -r <int>   minimum read length after trimming, default=" << Minimum_trimmed_read_len << endl;
	cout << "   -t <int>   number of threads to run, default=" << threadNum << endl;
	cout << "   -h         get help information" << endl;
	cout << "\nExample:\n  clean_adapter  -a Both-adapter -r 75 -s 12 sequencing_data_R1.fq.gz sequencing_data_R1.fq.nonAdapter.gz "
	        "sequencing_data_R1.fq.nonAdapter.stat\n" << endl;
	exit(0);
}

// alphabet[] of clean_adapter.cpp:54-64 (bytes from 128 on count as 4)
static int base_code(char ch)
{
	switch (ch) {
		case 'A': case 'a': return 0;
		case 'C': case 'c': return 1;
		case 'G': case 'g': return 2;
		case 'T': case 't': return 3;
		default: return 4;
	}
}

// read_fasta (clean_adapter.cpp:234-268): the id is the header up to its first blank, white space inside the sequence is removed,
// with -b 1 every sequence is followed by its reverse complement
static void read_fasta(const string &file_name, vector<string> &seqs, vector<string> &ids)
{
	ifstream infile(file_name.c_str(), ios::in);
	if (!infile) {
		cerr << "fail to open input file: " << file_name << endl;
		exit(-1);
	}
	string textline;
	getline(infile, textline, '>');
	while (getline(infile, textline, '\n')) {
		const string id = textline.substr(0, textline.find_first_of(" \t"));
		getline(infile, textline, '>');
		string purestr;
		for (char ch : textline)
			if (ch != '\n' && ch != ' ' && ch != '\t') purestr.push_back(ch);
		seqs.push_back(purestr);
		ids.push_back(id);
		if (Also_use_adapterRC == 1) {
			string rc_str;
			for (size_t i = purestr.size(); i-- > 0;) rc_str.push_back("TGCAN"[base_code(purestr[i])]);
			seqs.push_back(rc_str);
			ids.push_back(id + " minus-strand");
		}
	}
}

// what the program appends to a record's header (clean_adapter.cpp:189-220): the hit, if there is one, and the mark of a read that
// is shorter than -r after the cut.  Both routes call it.
static void adapter_suffix(const dbgk_adapter_hit &h, const vector<string> &ids, bool is_short, string &out)
{
	if (h.adapter >= 0) {
		out += "   Aligned to adapter " + ids[h.adapter] + ", ";
		out += " reads_pos: " + to_string(h.read_start) + "-" + to_string(h.read_end) + ", ";
		out += "adapter_pos: " + to_string(h.adapter_start) + "-" + to_string(h.adapter_end) + ", ";
		out += "  score: " + to_string(h.score);
	}
	if (is_short) out += "   RemoveShort";
}

static string default_adapter_file(const char *name)
{
	const char *dir = getenv("DBGK_ADAPTER_DIR");
	if (dir && *dir) {
		const string in_dir = string(dir) + "/" + name;
		if (ifstream(in_dir.c_str())) return in_dir;
	}
	return string("/qdata1/public/software/install/clean_illumina/") + name;
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "s:r:a:b:t:h")) != -1) {
		switch (c) {
			case 's': Alignment_score_cutoff = atoi(optarg); break;
			case 'r': Minimum_trimmed_read_len = atoi(optarg); break;
			case 'a': illumina_adapter_file = optarg; break;
			case 'b': Also_use_adapterRC = atoi(optarg); break;
			case 't': threadNum = atoi(optarg); break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 4 || argc - optind < 3) usage();
	if (Alignment_score_cutoff < 1) {
		cerr << "the minimum alignment score (-s) must be at least 1" << endl;
		return 1;
	}
	const string in_reads1_file = argv[optind++];
	const string out_reads1_file = argv[optind++];
	const string out_stat_file = argv[optind++];

	cerr << "\nAlignment score cutoff: " << Alignment_score_cutoff << endl;
	cerr << "Minimum trimmed read length: >=" << Minimum_trimmed_read_len << endl;
	const clock_t time_start = clock();

	if (illumina_adapter_file == "Both-adapter") illumina_adapter_file = default_adapter_file("illumina_NEB_adapter.fa");
	else if (illumina_adapter_file == "R1-adapter") illumina_adapter_file = default_adapter_file("illumina_NEB_adapter_R1.fa");
	else if (illumina_adapter_file == "R2-adapter") illumina_adapter_file = default_adapter_file("illumina_NEB_adapter_R2.fa");
	cerr << "\nLoad adapter sequences from " << illumina_adapter_file << endl;
	vector<string> AdapterVec, AdapterVecId;
	read_fasta(illumina_adapter_file, AdapterVec, AdapterVecId);
	for (size_t i = 0; i < AdapterVec.size(); i++) cerr << "Used illumina adapter: " << AdapterVecId[i] << " :   " << AdapterVec[i] << endl;
	if (AdapterVec.empty()) {
		cerr << "Died because illumina_adapter_file does not exist or no contamination sequences are provided\n";
		exit(0);
	}
	cerr << "\nInput Reads  file:  " << in_reads1_file << endl << endl;

	dbgk_clean *cleaner = nullptr;
	int rc = dbgk_clean_create(0, &cleaner);
	if (rc) die("dbgk_clean_create", rc);
	string bases;
	vector<uint64_t> offsets;
	concat(AdapterVec, bases, offsets);
	rc = dbgk_clean_set_adapters(cleaner, bases.data(), offsets.data(), AdapterVec.size(), Alignment_score_cutoff);
	if (rc) die("dbgk_clean_set_adapters", rc);

	uint64_t total_raw_reads = 0, total_raw_bases = 0, total_clean_reads = 0, total_clean_bases = 0;
	uint64_t total_adapter_trimmed_reads = 0, total_adapter_trimmed_bases = 0, total_Nmasked_short_reads = 0, total_Nmasked_short_bases = 0;
	if (text_on_device()) {
		GzWriter cleanfile1(out_reads1_file);
		DeviceTextTotals T;
		vector<dbgk_adapter_hit> hits;
		clean_text_on_device(in_reads1_file, cleanfile1, cleaner, Minimum_trimmed_read_len, true, T,
		                     [&](const char *d_bases, const char *d_quals, const uint64_t *offsets, const uint64_t *lens, uint64_t n, string &suffix,
		                         vector<uint64_t> &suffix_offsets) {
			hits.resize(n + 1);
			const int rc = dbgk_clean_adapter_device(cleaner, d_bases, d_quals, offsets, n, hits.data());
			if (rc) die("dbgk_clean_adapter_device", rc);
			for (uint64_t i = 0; i < n; i++) {
				const dbgk_adapter_hit &h = hits[i];
				const uint64_t kept = h.adapter >= 0 ? min<uint64_t>(lens[i], (uint64_t)(h.read_start - 1)) : lens[i];
				adapter_suffix(h, AdapterVecId, kept < (uint64_t)Minimum_trimmed_read_len, suffix);
				suffix_offsets.push_back(suffix.size());
			}
		});
		cleanfile1.close();
		total_raw_reads = T.raw_reads, total_raw_bases = T.raw_bases;
		total_adapter_trimmed_reads = T.trimmed_reads, total_adapter_trimmed_bases = T.trimmed_bases;
		total_Nmasked_short_reads = T.short_reads, total_Nmasked_short_bases = T.short_bases;
		total_clean_reads = T.clean_reads, total_clean_bases = T.clean_bases;
	} else {
		LineReader infile1(in_reads1_file);
		GzWriter cleanfile1(out_reads1_file);
		RecordBatch batch;
		vector<dbgk_adapter_hit> hits;
		for (bool more = true; more;) {
			more = batch.fill(infile1, total_raw_reads, total_raw_bases);
			cerr << "reading num " << batch.size() << endl;
			concat(batch.reads, bases, offsets);
			hits.resize(batch.size() + 1);
			rc = dbgk_clean_adapter(cleaner, bases.data(), offsets.data(), batch.size(), hits.data());
			if (rc) die("dbgk_clean_adapter", rc);
			for (size_t i = 0; i < batch.size(); i++) { // thread_trimReads (clean_adapter.cpp:189-220)
				const dbgk_adapter_hit &h = hits[i];
				string &read = batch.reads[i];
				if (h.adapter >= 0) {
					const int read_len = (int)read.size();
					const int trimmed_read_len = h.read_start - 1;
					read = read.substr(0, trimmed_read_len);
					batch.quals[i] = batch.quals[i].substr(0, trimmed_read_len);
					total_adapter_trimmed_reads++;
					total_adapter_trimmed_bases += read_len - h.read_start + 1;
				}
				const bool is_short = read.size() < (size_t)Minimum_trimmed_read_len;
				adapter_suffix(h, AdapterVecId, is_short, batch.heads[i]);
				if (is_short) {
					total_Nmasked_short_reads++;
					total_Nmasked_short_bases += read.size();
					read = "";
					batch.quals[i] = "";
				} else {
					total_clean_reads++;
					total_clean_bases += read.size();
				}
			}
			batch.write(cleanfile1);
			batch.clear();
		}
		cleanfile1.close();
	}
	dbgk_clean_destroy(cleaner);

	ofstream statfile(out_stat_file.c_str());
	statfile << "total_raw_reads:  " << total_raw_reads << endl;
	statfile << "total_raw_bases:  " << total_raw_bases << endl;
	const double adapter_ratio = (double)total_adapter_trimmed_bases / total_raw_bases;
	statfile << "total_adapter_trimmed_reads:  " << total_adapter_trimmed_reads << endl;
	statfile << "total_adapter_trimmed_bases:  " << total_adapter_trimmed_bases << "\t" << adapter_ratio << endl;
	const double Nmasked_ratio = (double)total_Nmasked_short_bases / total_raw_bases;
	statfile << "total_short_trimmed_reads:  " << total_Nmasked_short_reads << endl;
	statfile << "total_short_trimmed_bases:  " << total_Nmasked_short_bases << "\t" << Nmasked_ratio << endl;
	const double clean_ratio = (double)total_clean_bases / total_raw_bases;
	statfile << "total_clean_reads:  " << total_clean_reads << endl;
	statfile << "total_clean_bases:  " << total_clean_bases << "\t" << clean_ratio << endl;

	cerr << "\nAll jobs finished\n";
	cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl;
	return 0;
}
